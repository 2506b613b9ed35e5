"""kmws_reframe_utf8_batch / kmws_unpack_reframe_utf8 on the device.  Every run
asserts four things:
  1. dst (the whole pre-filled buffer), wire_off and the status are bit-equal to
     kmws_reframe_batch / kmws_unpack_reframe on the same inputs;
  2. src is unchanged;
  3. out_utf8[:n] and carry_out equal kmws_utf8_validate(payload_masked = 1) on
     the plain reframe's output wire with, for an emitted frame, D[i] =
     {wire_off[i] + header length, len, outgoing key if masked else 0} and F[i] =
     flags[i] & 0x1FF, for a skipped frame D[i] = {wire_off[i], 0, 0}, F[i] = 0x89;
  4. out_utf8 equals tests/utf8_ref.py applied to the emitted frames, NOT_TEXT
     scattered into the skipped ones.
Every case runs in both copy forms (chunks below 16 KiB of dst_cap per frame,
units from it, chosen by dst_cap alone) and with the outgoing frames unmasked
and masked with fresh keys.  All comparisons are exact."""
import functools
import random

import numpy as np
import pytest

import test_gpu_reframe as rf
import test_gpu_utf8 as vt
import utf8_ref as ref
from test_gpu_utf8 import B_, C_, FIN, PING, RSV1, T_, Batch

FILL = 0xAB
FORMS = ("chunk", "unit")
KINDS = ("unmasked", "masked")
UNIT_FROM = 16384  # dst_cap / n from which the unit form runs
SKIP, MASK = 0x8000, 0x100
CHUNK = 4096


def hdr_len(lens, masked):
    lens = np.asarray(lens, dtype=np.int64)
    return np.where(lens <= 125, 2, np.where(lens <= 65535, 4, 10)) + (4 if masked else 0)


def r16(x):
    return (x + 15) // 16 * 16


def both_forms(frames):
    """The frames, with empty PING frames appended until the mean region (14
    header bytes at most) is below the unit form's threshold: then dst_cap alone
    selects the form."""
    frames = list(frames)
    total = sum(len(p) for _, p in frames)
    while frames and (r16(total + 14 * len(frames)) + 16) // len(frames) >= UNIT_FROM:
        frames.append((PING | FIN, b""))
    return frames


def dst_cap_of(form, n, total):
    tight = r16(total) + 16
    cap = tight if form == "chunk" else max(UNIT_FROM * n, tight)
    if n:
        assert (cap // n < UNIT_FROM) == (form == "chunk"), (form, n, total)
    return cap


def out_keys_for(n, seed):
    keys = np.random.default_rng(0x0C0FFEE + seed).integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[5::13] = 0  # a masked frame whose key is 0
    return keys


def want_emitted(frames, skip, stream_first=None):
    """utf8_ref on the emitted frames of each stream, NOT_TEXT in the skipped ones."""
    n = len(frames)
    first = [0, n] if stream_first is None else [int(x) for x in stream_first]
    out = np.full(n, ref.NOT_TEXT, dtype=np.uint8)
    for a, b in zip(first, first[1:]):
        idx = [i for i in range(a, b) if not skip[i]]
        if idx:
            out[idx] = ref.validate_stream([frames[i] for i in idx])[0]
    return out


def i16(a):
    import torch as T
    return T.from_numpy(np.asarray(a).astype(np.uint16).view(np.int16)).cuda()


def validate_output_wire(dst, off, n, lens, hl, sk, masked, okeys, fl, ns, sf, ci):
    """(3): kmws_utf8_validate on the finished output wire with D / F."""
    import torch as T
    from kuma_amd import kmws
    total = int(off[n].item())
    o = off[:n].cpu().numpy()
    D = kmws.make_descs(np.where(sk, o, o + hl), np.where(sk, 0, lens),
                        np.where(sk | (not masked), 0, okeys).astype(np.int64))
    F = i16(np.where(sk, 0x89, fl & 0x1FF))
    out = T.full((max(n, 1),), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((max(ns, 1), 8), 0xEE, dtype=T.uint8, device="cuda")
    wv = kmws.Workspace(kmws.utf8_workspace_size(total, n, ns))
    kmws.utf8_validate(dst, D, F, out, wv, span=total, masked=True, stream_first=sf, carry_in=ci, carry_out=co)
    assert wv.status() == 0
    return out, co


def run_reframe(batch, kind, form, skip=None, wild=False, stream_first=None, carry_in=None, lo=0, hi=None, cap=None,
                seed=0):
    """Frames [lo, hi) of the batch through the fused call, the plain reframe and
    kmws_utf8_validate on the plain reframe's output; asserts 1-3 of the module's
    contract and returns (verdicts, carry_out)."""
    import torch as T
    from kuma_amd import kmws
    hi = batch.n if hi is None else hi
    n = hi - lo
    masked = kind == "masked"
    lens = batch.lens[lo:hi].astype(np.int64)
    offs = batch.offs[lo:hi].astype(np.int64).copy()
    sk = np.zeros(n, dtype=bool) if skip is None else np.asarray(skip, dtype=bool)[lo:hi]
    fl = (batch.flags[lo:hi] & 0xFF) | (MASK if masked else 0) | np.where(sk, SKIP, 0)
    okeys = out_keys_for(batch.n, seed)[lo:hi]
    dlens = lens.copy()
    if wild:  # skipped frames pointing far outside src: never used for an address
        offs[sk] = (1 << 46) + 977 * np.arange(int(sk.sum()))
        dlens[sk] = np.resize(np.array([0xFFFFFFFF, 1 << 31, 70000, 4096, 126, 1], dtype=np.int64), int(sk.sum()))
    hl = np.where(sk, 0, hdr_len(lens, masked))
    want_off = np.concatenate([[0], np.cumsum(np.where(sk, 0, hl + lens))]).astype(np.int64)
    total = int(want_off[-1])
    cap = dst_cap_of(form, n, total) if cap is None else cap
    host_src = batch.masked()
    src = T.from_numpy(host_src).cuda()
    descs = kmws.make_descs(offs, dlens, batch.keys[lo:hi].astype(np.int64))
    d_fl = i16(fl)
    d_ok = T.from_numpy(okeys.view(np.int32).copy()).cuda()
    ns = 1 if stream_first is None else len(stream_first) - 1
    sf = None if stream_first is None else T.tensor(list(stream_first), dtype=T.int32, device="cuda")
    ci = None if carry_in is None else T.from_numpy(np.ascontiguousarray(carry_in, dtype=np.uint8)).cuda()
    res = {}
    for fused in (True, False):
        dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        out = T.full((max(n, 1),), 0xEE, dtype=T.uint8, device="cuda")
        co = T.full((max(ns, 1), 8), 0xEE, dtype=T.uint8, device="cuda")
        if fused:
            ws = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap, ns))
            kmws.reframe_utf8(src, descs, d_fl, d_ok, dst, off, out, ws, stream_first=sf, carry_in=ci, carry_out=co)
        else:
            ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
            kmws.reframe_batch(src, descs, d_fl, d_ok, dst, off, ws)
        assert ws.status() == 0, (kind, form, fused)
        if not fused and n:
            out, co = validate_output_wire(dst, off, n, lens, hl, sk, masked, okeys, fl, ns, sf, ci)
        res[fused] = (dst, off, out, co)
    assert np.array_equal(src.cpu().numpy(), host_src), "src was written"
    (dst, off, out, co), (dst2, off2, out2, co2) = res[True], res[False]
    tag = (kind, form, n)
    assert T.equal(off, off2) and np.array_equal(off.cpu().numpy(), want_off), tag
    assert T.equal(dst, dst2), tag + (rf.first_true(dst != dst2),)  # the bytes, and the fill past the total
    assert bool((dst[total:] == FILL).all()), tag
    if n:
        assert T.equal(co, co2), tag + (co.cpu().numpy(), co2.cpu().numpy())
        assert T.equal(out[:n], out2[:n]), tag + (T.nonzero(out[:n] != out2[:n])[:8].cpu().numpy(),)
    return out.cpu().numpy()[:n], co.cpu().numpy()[:ns]


def check(batch, expect=None, skip=None, forms=FORMS, kinds=KINDS, **kw):
    sk = np.zeros(batch.n, dtype=bool) if skip is None else np.asarray(skip, dtype=bool)
    if expect is None:
        expect = want_emitted(batch.frames, sk, kw.get("stream_first"))
    expect = np.asarray(expect, dtype=np.uint8)
    for kind in kinds:
        for form in forms:
            out, _ = run_reframe(batch, kind, form, skip=sk, **kw)
            bad = np.nonzero(out != expect)[0]
            assert bad.size == 0, (kind, form, bad[:10], out[bad[:10]], expect[bad[:10]])
    return expect


def packed(frames, seed=1):
    offs, total = vt.packed_offsets([len(p) for _, p in frames], random.Random(seed))
    return Batch(frames, offs, total, seed=seed)


# ---------------------------------------------------------------- 1. known answers

@pytest.mark.gpu
def test_known_answers():
    frames, expect = [], []
    for data, ok in vt.KNOWN:
        frames += [(T_ | FIN, data), (B_ | FIN, data), (T_ | FIN | RSV1, data)]
        expect += [ref.OK if ok else ref.BAD, ref.NOT_TEXT, ref.NOT_TEXT]
    assert list(vt.want(frames)) == expect
    check(packed(frames), expect)


# ---------------------------------------------------------------- 2. boundary sweep in output space

# (unit of dst, how many of its multiples from the payload's first byte on): the 16-byte word, the
# 64-byte ownership granule, a wave-instruction's 1 KiB row, a 4 KiB unit / chunk
OUT_CLASSES = ((16, 4), (64, 4), (1024, 8), (4096, 4))


@functools.lru_cache(maxsize=None)
def sweep_texts():
    """The sweep text cut to 20 KiB (header forms 4 / 8) and doubled (80 KiB: 10 / 14)."""
    data, _ = vt.sweep_text()
    cut = 20 * 1024
    while (data[cut] & 0xC0) == 0x80:
        cut += 1
    mid, big = data[:cut], data + data
    assert ref.valid(mid) and ref.valid(big) and len(big) >= 65536
    return mid, big


def sweep_cands(arr, off):
    """Corruptions (class unit, p, new byte) of a copy of arr whose payload lies
    at dst offset off, with off + p within +-4 bytes of a multiple of the unit."""
    seen, res = set(), []
    for unit, count in OUT_CLASSES:
        m0 = (off + unit - 1) // unit * unit
        for k in range(count):
            for dlt in range(-4, 5):
                p = m0 + k * unit + dlt - off
                if not 0 <= p < len(arr) or p in seen:
                    continue
                seen.add(p)
                res.append((unit, p, 0xFF))
                width = 2 if 0xC2 <= arr[p] <= 0xDF else 3 if 0xE0 <= arr[p] <= 0xEF else 4 if arr[p] >= 0xF0 else 0
                if width and p + width <= len(arr):
                    res.append((unit, p + width - 1, 0x61))  # truncated: its last continuation becomes "a"
    return res


SHORT = ("a€😀" * 15).encode()  # 120 bytes: header forms 2 / 6


def sweep_frames(r, masked):
    """A sweep batch whose first copy's payload lies at phase r of dst mod 16.
    r % 3 == 0: 20 KiB copies, each with the next corruption of its own offset's
    list; == 1: 120-byte copies behind binary fillers sized so that the
    corrupted byte lies at each offset of every class's multiple; == 2: 80 KiB
    copies, every third corruption.  Returns (frames, expected verdicts, header
    lengths seen, payload phases seen, classes hit)."""
    mid, big = sweep_texts()
    m = 4 if masked else 0
    frames, expect, hls, phases, classes = [], [], set(), set(), {}
    cur = 0  # dst offset of the next frame

    def emit(b0, payload, verdict):
        nonlocal cur
        hl = int(hdr_len(len(payload), masked))
        hls.add(hl)
        if (b0 & 0x0F) == T_:
            phases.add((cur + hl) % 16)
        frames.append((b0, payload))
        expect.append(verdict)
        cur += hl + len(payload)
        return cur - len(payload)

    if r % 3 == 1:
        hf, ht = 4 + m, 2 + m  # the fillers' header (126..65535 bytes) and the texts'
        filler = lambda L: bytes(0x80 + (i % 0x80) for i in range(L))  # noqa: E731
        emit(B_ | FIN, filler(126 + ((r - (cur + hf + 126 + ht)) % 16)), ref.NOT_TEXT)
        assert emit(T_ | FIN, SHORT, ref.OK) % 16 == r  # the first text payload at phase r
        for unit, _ in OUT_CLASSES:
            for dlt in range(-4, 5):
                for trunc in (False, True):
                    # "a" at 56, "€" at 57..59, the emoji at 60..63: its lead becomes FF, or its last byte "a"
                    p = 63 if trunc else 60
                    # the filler: the text's corrupted byte p lands dlt past a multiple of the unit
                    emit(B_ | FIN, filler(126 + ((dlt - (cur + hf + 126 + ht + p)) % unit)), ref.NOT_TEXT)
                    body = bytearray(SHORT)
                    body[p] = 0x61 if trunc else 0xFF
                    i_bad, _ = ref.first_bad(bytes(body))
                    assert i_bad is not None
                    at = emit(T_ | FIN, bytes(body), ref.BAD)
                    assert (at + p - dlt) % unit == 0
                    classes[unit] = classes.get(unit, 0) + 1
        return frames, expect, hls, phases, classes
    text = big if r % 3 == 2 else mid
    arr = np.frombuffer(text, dtype=np.uint8)
    stride = 3 if r % 3 == 2 else 1
    ht = int(hdr_len(len(text), masked))
    fill = (r - (2 + m) - ht) % 16  # a short binary frame: the first copy's payload at phase r
    emit(B_ | FIN, bytes(range(0x80, 0x80 + fill)), ref.NOT_TEXT)
    emit(T_ | FIN, text, ref.OK)
    ncopies = len(sweep_cands(arr, r)) // stride
    for j in range(ncopies):
        cands = sweep_cands(arr, cur + ht)
        unit, p, newb = cands[(j * stride) % len(cands)]
        body = bytearray(text)
        body[p] = newb
        emit(T_ | FIN, bytes(body), vt.sweep_verdict(np.frombuffer(bytes(body), dtype=np.uint8), p))
        classes[unit] = classes.get(unit, 0) + 1
    return frames, expect, hls, phases, classes


def test_sweep_covers_every_phase_and_header_form():
    """CPU: over the parameters the payload's phase in dst takes all 16 values
    and the header all six lengths; every parameter hits every boundary class."""
    hls, phases = set(), set()
    for r in range(16):
        for masked in (False, True):
            frames, expect, h, ph, classes = sweep_frames(r, masked)
            assert r in ph, (r, masked, ph)
            assert all(classes.get(u, 0) >= 1 for u, _ in OUT_CLASSES), classes
            assert ref.BAD in expect
            hls |= h
            phases |= ph
    assert hls >= {2, 4, 10, 6, 8, 14} and phases == set(range(16))


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(16))
def test_boundary_sweep_in_output_space(r):
    # src offset mod 16: the first copy's phase in dst and three that differ from it, dealt over the two kinds
    phases = {"unmasked": (r, (r + 7) % 16), "masked": ((r + 1) % 16, (r + 12) % 16)}
    for kind in KINDS:
        frames, expect, _, _, _ = sweep_frames(r, kind == "masked")
        frames = both_forms(frames)
        expect = expect + [ref.NOT_TEXT] * (len(frames) - len(expect))
        for s in phases[kind]:
            offs, pos = [], 0
            for _, p in frames:
                pos = r16(pos) + 16 + s
                offs.append(pos)
                pos += len(p)
            check(Batch(frames, offs, pos + 5, seed=r), expect, kinds=(kind,))


# ---------------------------------------------------------------- 3. fragment straddles

@pytest.mark.gpu
def test_fragment_straddles():
    rng = random.Random(7)
    frames = vt.straddle_frames(rng)
    pings = [i for i, (b0, p) in enumerate(frames) if (b0 & 0x0F) == PING and p]
    skip = np.zeros(len(frames), dtype=bool)
    skip[pings[1::2]] = True  # every second PING is dropped, the others are relayed between the halves
    expect = want_emitted(frames, skip)
    assert np.array_equal(expect, vt.want(frames))  # a control frame is invisible either way
    assert set(expect) == {0, 1, 2, 3}
    assert any(b0 == (C_ | FIN) and p == b"" and e == ref.BAD for (b0, p), e in zip(frames, expect))
    assert any(b0 == C_ and p == b"" for b0, p in frames)
    assert skip.any() and any(not skip[i] for i in pings)
    check(packed(frames, 7), expect, skip=skip, wild=True)


@pytest.mark.gpu
@pytest.mark.parametrize("top", [1, 3], ids=["dense_0_1", "frames_0_to_3"])
def test_tiny_fragments_across_scan_tiles(top):
    """n = 3 * 2048 + 7 frames of 0..top bytes: every code point straddles
    fragments with header bytes between its halves, a 4 KiB chunk holds far more
    than 64 frames (chunk_dense_kernel), the chunk scan's look-back crosses its
    2048-frame tiles and the UTF-8 scan its 256-frame blocks."""
    n = 3 * 2048 + 7
    lens = np.random.default_rng(50 + top).integers(0, top + 1, size=n)
    frames = vt.fill_messages(lens, 60 + top)
    assert 4096 // (max(int(lens.sum()) // n, 1) + 6) > 64
    expect = vt.want(frames)
    assert {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD} <= set(expect)
    check(packed(frames, 51), expect)


# ---------------------------------------------------------------- 4. skips are invisible

@pytest.mark.gpu
def test_skipped_head_and_skipped_middle_fragment():
    euro = "€".encode()
    frames = [(T_, b"ab"), (C_, b"cd"), (C_ | FIN, b"ef"),            # head skipped: the CONTINUEs belong to nothing
              (T_, euro[:1]), (C_, b"\xff\xff"), (C_ | FIN, euro[1:]),  # middle skipped: its neighbours join to "€"
              (T_, euro[:1]), (C_, b"\xff\xff"), (C_ | FIN, euro[1:]),  # the same, nothing skipped: BAD
              (T_ | FIN, b"ok")]
    skip = np.zeros(len(frames), dtype=bool)
    skip[[0, 4]] = True
    expect = want_emitted(frames, skip)
    assert list(expect) == [0, 0, 0, 1, 0, 1, 1, 2, 3, 1]
    check(packed(frames, 3), expect, skip=skip, wild=True)


SKIP_PATTERNS = ("every_third", "run65_on_chunk_boundary", "whole_scan_tile", "last_frames")


@functools.lru_cache(maxsize=None)
def skip_frames():
    n = 2 * 2048 + 300
    rng = np.random.default_rng(77)
    lens = rng.choice([0, 1, 3, 17, 100, 125, 126, 300, 1000, 4096], size=n, p=[.05, .05, .1, .1, .2, .1, .1, .2, .05, .05])
    return vt.fill_messages(lens, 78)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", SKIP_PATTERNS)
def test_skips_are_invisible(pattern):
    base = skip_frames()
    n = len(base)
    for kind in KINDS:
        frames = list(base)
        skip = np.zeros(n, dtype=bool)
        if pattern == "every_third":
            skip[::3] = True
        elif pattern == "run65_on_chunk_boundary":
            j = n // 3
            skip[j:j + 65] = True
            # frame j - 1 becomes a binary filler that ends on a 4 KiB boundary of dst
            m = kind == "masked"
            lens = np.array([len(p) for _, p in frames[:j - 1]], dtype=np.int64)
            at = int((hdr_len(lens, m) + lens).sum()) + 4 + (4 if m else 0)
            frames[j - 1] = (B_ | FIN, bytes(126 + (-(at + 126)) % CHUNK))
            lens = np.array([len(p) for _, p in frames[:j]], dtype=np.int64)
            assert int((hdr_len(lens, m) + lens).sum()) % CHUNK == 0
        elif pattern == "whole_scan_tile":
            skip[2048:4096] = True
        else:
            skip[n - 77:] = True
        expect = want_emitted(frames, skip)
        assert {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD} <= set(expect)
        assert not np.array_equal(expect, vt.want(frames))  # the skips change verdicts
        check(packed(frames, 79), expect, skip=skip, kinds=(kind,), wild=True)


# ---------------------------------------------------------------- 5. streams and carry

def stream_skips(b):
    skip = np.zeros(b.n, dtype=bool)
    skip[7::11] = True
    return skip


@pytest.mark.gpu
def test_streams_in_one_call():
    b, first, expect = vt.stream_batch()
    assert any(first[s] == first[s + 1] for s in range(len(first) - 1))  # empty streams
    check(b, expect, stream_first=first)
    skip = stream_skips(b)
    check(b, want_emitted(b.frames, skip, first), skip=skip, stream_first=first)


@pytest.mark.gpu
def test_streams_cut_into_two_calls_joined_by_the_carry():
    b, first, expect = vt.stream_batch()
    assert ref.AFTER_BAD in expect
    s5, s6, s8 = (int(first[s]) for s in (5, 6, 8))
    # s6: a message already BAD carried across the cut (AFTER_BAD behind it)
    assert list(expect[s6:s6 + 4]) == [ref.BAD, ref.NOT_TEXT, ref.AFTER_BAD, ref.AFTER_BAD]
    for c in (s5 + 1, s5 + 2, s6 + 1, s6 + 3, s8 + 1, int(first[21]), b.n // 2):
        f1 = np.minimum(first, c)
        f2 = np.maximum(first, c) - c
        for kind in KINDS:
            for form in FORMS:
                out1, carry = run_reframe(b, kind, form, stream_first=f1, lo=0, hi=c)
                out2, _ = run_reframe(b, kind, form, stream_first=f2, carry_in=carry, lo=c)
                assert np.array_equal(out2, expect[c:]), (c, kind, form, np.nonzero(out2 != expect[c:])[0][:10])
                assert np.array_equal(out1, expect[:c]), (c, kind, form)


@pytest.mark.gpu
@pytest.mark.parametrize("second", [vt.OK_PIECE, vt.BAD_PIECE], ids=["ok", "bad"])
def test_message_open_across_rounds(second):
    """tests/test_gpu_utf8.py's round-two case through the fused reframe: the
    frame state crosses the first round of the aggregate scan (run_reframe checks
    the output wire and the offsets as ever)."""
    frames, at = vt.round_edge_frames(*vt.EDGE_ROUNDS[2], second)
    expect = vt.round_edge_expect(frames, at, second)
    out, carry = run_reframe(vt.round_edge_batch(frames), "masked", "chunk")
    bad = np.nonzero(out != expect)[0]
    assert bad.size == 0, (bad[:10], out[bad[:10]], expect[bad[:10]])
    assert bytes(carry[0]) == vt.scan_carry_after(frames, expect, bytes(8))


# ---------------------------------------------------------------- 6. contract

def small_batch():
    frames = [(T_ | FIN, b"abc"), (T_ | FIN, "€".encode()), (T_ | FIN, b"\xff"), (T_ | FIN, b"z" * 40)]
    return Batch(frames, [4, 20, 40, 60], 128)


def raw_call(b, cap, stream_first=None, n=None, carry_in=None):
    """The entry on its own buffers: (status, dst, wire_off, carry_out)."""
    import torch as T
    from kuma_amd import kmws
    n = b.n if n is None else n
    src = T.from_numpy(b.masked()).cuda()
    descs = kmws.make_descs(b.offs[:n], b.lens[:n], b.keys[:n].astype(np.int64))
    fl = i16((b.flags[:n] & 0xFF) | MASK)
    ok = T.from_numpy(out_keys_for(b.n, 1)[:n].view(np.int32).copy()).cuda()
    ns = 1 if stream_first is None else len(stream_first) - 1
    sf = None if stream_first is None else T.tensor(list(stream_first), dtype=T.int32, device="cuda")
    ci = None if carry_in is None else T.from_numpy(np.ascontiguousarray(carry_in, dtype=np.uint8)).cuda()
    dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
    off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    out = T.full((max(n, 1),), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((ns, 8), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap, ns))
    kmws.reframe_utf8(src, descs, fl, ok, dst, off, out, ws, stream_first=sf, carry_in=ci, carry_out=co)
    return ws.status(), dst.cpu().numpy(), off.cpu().numpy(), co.cpu().numpy()


@pytest.mark.gpu
def test_contract_cap_streams_and_empty_batch():
    good = small_batch()
    assert list(check(good)) == [1, 1, 2, 1]
    total = int((good.lens + 6).sum())
    # total > dst_cap: status bit 1, nothing stored -- the chunk form, then the unit form
    st, dst, _, _ = raw_call(good, 32)
    assert st & 1 and (dst == FILL).all()
    big = Batch([(T_ | FIN, b"q" * 20000)] * 3, [16, 20032, 40048], 60064)
    assert UNIT_FROM * 3 < 60000
    st, dst, _, _ = raw_call(big, UNIT_FROM * 3)
    assert st & 1 and (dst == FILL).all()
    for form in FORMS:
        cap = dst_cap_of(form, good.n, total)
        for sf in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3], [0, 5, 4]):  # malformed: bit 1, nothing stored
            st, dst, _, _ = raw_call(good, cap, stream_first=sf)
            assert st & 1 and (dst == FILL).all(), (form, sf)
        st, dst, off, _ = raw_call(good, cap, stream_first=[0, 0, 2, 2, 4, 4])
        assert st == 0 and off[-1] == total
    # n == 0: OK, wire_off[0] = 0, carry_out = carry_in
    carry = np.arange(24, dtype=np.uint8).reshape(3, 8)
    st, dst, off, co = raw_call(good, 64, stream_first=[0, 0, 0, 0], n=0, carry_in=carry)
    assert st == 0 and off[0] == 0 and np.array_equal(co, carry) and (dst == FILL).all()
    out, co = run_reframe(good, "masked", "chunk", lo=0, hi=0, cap=64)
    assert out.size == 0 and np.array_equal(co, np.zeros((1, 8), dtype=np.uint8))


# ---------------------------------------------------------------- 7. the unpack form

def unpack_call(T, fused, d_wire, W, d_hdr, mode, relay, out_mask, d_ok, cap):
    from kuma_amd import kmws
    n = d_hdr.shape[0]
    buf, dst = rf.guarded(T, cap)
    off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    fd = T.full((n, 2), -1, dtype=T.int64, device="cuda")
    ff = T.full((n,), -1, dtype=T.int16, device="cuda")
    fe = T.full((n,), 99, dtype=T.uint8, device="cuda")
    out = T.full((n,), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((1, 8), 0xEE, dtype=T.uint8, device="cuda")
    if fused:
        ws = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap, 1))
        kmws.unpack_reframe_utf8(d_wire, d_hdr, mode, fd, ff, fe, relay, out_mask, d_ok, dst, off, out, ws, wire_len=W,
                                 carry_out=co)
    else:
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.unpack_reframe(d_wire, d_hdr, mode, fd, ff, fe, relay, out_mask, d_ok, dst, off, ws, wire_len=W)
    return buf, dst, off, fd, ff, fe, out, co, ws.status()


@pytest.mark.gpu
@pytest.mark.parametrize("relay", (0x0007, 0xFFFF))
@pytest.mark.parametrize("errors", (False, True), ids=("clean", "errors"))
@pytest.mark.parametrize("mode", (rf.hc.SERVER, rf.hc.CLIENT), ids=("server", "client"))
def test_unpack_reframe_utf8(mode, errors, relay):
    import torch as T
    wire, hdr_off, e, nbad = rf.relay_wire(mode, errors)
    wire = wire.copy()
    n = len(hdr_off)
    # text the check can pass: the payloads of half the frames become (masked) ASCII
    for i in range(0, n, 2):
        if e.err[i] == 0 and e.len[i]:
            a, L = int(e.off[i]), int(e.len[i])
            kb = np.frombuffer(np.uint32(e.key[i]).tobytes(), dtype=np.uint8)
            wire[a:a + L] = (0x61 + np.arange(L) % 26).astype(np.uint8) ^ np.tile(kb, L // 4 + 1)[:L]
    skip = (e.err != 0) | (((relay >> (e.flags & 0x0F)) & 1) == 0)
    frames = []
    for i in range(n):
        a, L = int(e.off[i]), int(e.len[i])
        kb = np.frombuffer(np.uint32(e.key[i]).tobytes(), dtype=np.uint8)
        frames.append((int(e.flags[i]) & 0xFF, b"" if skip[i] else bytes(wire[a:a + L] ^ np.tile(kb, L // 4 + 1)[:L])))
    expect = want_emitted(frames, skip)
    assert {ref.NOT_TEXT, ref.OK, ref.BAD} <= set(expect)
    out_keys = out_keys_for(n, relay + mode)
    d_wire = rf.to_dev(T, wire)
    d_hdr = T.from_numpy(hdr_off).cuda()
    d_ok = T.from_numpy(out_keys.view(np.int32).copy()).cuda()
    lens = e.len.astype(np.int64)
    for out_mask in (0, 1):
        hl = np.where(skip, 0, hdr_len(lens, out_mask))
        total = int(np.where(skip, 0, hl + lens).sum())
        oflags = (e.flags & 0xFF) | (MASK if out_mask else 0) | np.where(skip, SKIP, 0)
        for form in FORMS:
            cap = rf.cap_for("chunks" if form == "chunk" else "units", n, total)
            got = unpack_call(T, True, d_wire, len(wire), d_hdr, mode, relay, out_mask, d_ok, cap)
            two = unpack_call(T, False, d_wire, len(wire), d_hdr, mode, relay, out_mask, d_ok, cap)
            tag = (mode, errors, hex(relay), out_mask, form)
            assert got[8] == two[8] == (2 if nbad else 0), tag
            for name, a, b_ in zip(("buf", "dst", "wire_off", "out_desc", "out_flags", "out_err"), got, two):
                assert T.equal(a, b_), tag + (name,)
            assert int(got[2][n].item()) == total
            assert np.array_equal(d_wire[:len(wire)].cpu().numpy(), wire), "the wire was written"
            out3, co3 = validate_output_wire(two[1], two[2], n, lens, hl, skip, bool(out_mask), out_keys, oflags, 1,
                                             None, None)
            assert T.equal(got[6], out3[:n]) and T.equal(got[7], co3), tag
            assert np.array_equal(got[6].cpu().numpy(), expect), tag


# ---------------------------------------------------------------- 8. fuzz

FUZZ_BLOCKS = 4


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    rng = np.random.default_rng(0xF0227 + seed)
    n = int(rng.integers(1, 301))
    lens = rng.choice(rf.FUZZ_LENS, size=n).astype(np.int64)
    big = np.flatnonzero(lens >= 65535)
    lens[big[3:]] = rng.choice(rf.FUZZ_LENS[:24], size=len(big[3:]))  # at most three large frames: under 1 MiB
    frames = vt.fill_messages(lens, 500 + seed)  # opcodes, FIN, RSV1, control frames, corrupted text
    skip = np.zeros(n, dtype=bool)
    skip[rng.permutation(n)[:int(rng.integers(0, n // 4 + 1))]] = True
    return both_forms(frames), skip


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(FUZZ_BLOCKS))
def test_fuzz(block):
    seen = set()
    for seed in range(6 * block, 6 * block + 6):
        frames, skip = fuzz_case(seed)
        skip = np.concatenate([skip, np.zeros(len(frames) - len(skip), dtype=bool)])
        assert sum(len(p) for _, p in frames) <= 4 << 20
        b = packed(frames, 600 + seed)
        seen |= set(check(b, skip=skip, wild=True, seed=seed))
    assert seen == {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD}


# ---------------------------------------------------------------- 9. captured graph

@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_captured_graph_follows_the_payload(form):
    import torch as T
    from kuma_amd import kmws
    data = ref.text(random.Random(9), 50000)
    frames = both_forms([(T_ | FIN, data), (T_ | FIN, b"tail")])
    n = len(frames)
    b = Batch(frames, [6, 50020] + [0] * (n - 2), 50040)
    b.keys[:] = 0  # the payload is rewritten in place below: plain bytes
    total = int((hdr_len(b.lens, False) + b.lens).sum())
    cap = dst_cap_of(form, n, total)
    src = T.from_numpy(b.masked()).cuda()
    descs = kmws.make_descs(b.offs, b.lens, b.keys.astype(np.int64))
    fl = i16(b.flags & 0xFF)  # unmasked outgoing frames: dst holds the plain bytes
    dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
    off = T.zeros(n + 1, dtype=T.int64, device="cuda")
    out = T.full((n,), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap, 1))
    call = lambda: kmws.reframe_utf8(src, descs, fl, None, dst, off, out, ws)  # noqa: E731
    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(s):
        call()  # warm: every kernel loaded before the capture
    T.cuda.current_stream().wait_stream(s)
    T.cuda.synchronize()
    assert ws.status() == 0 and list(out.cpu().numpy()[:2]) == [1, 1]
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        call()
    T.cuda.synchronize()
    p = 33333
    for newb, verdict in ((0xFF, 2), (b.plain[6 + p], 1)):
        src[6 + p] = int(newb)
        out.fill_(0xEE)
        dst.fill_(FILL)
        g.replay()
        T.cuda.synchronize()
        assert ws.status() == 0
        assert list(out.cpu().numpy()[:2]) == [verdict, 1]
        assert int(dst[4 + p].item()) == int(newb) and bytes(dst[50004 + 2:50004 + 6].cpu().numpy()) == b"tail"
