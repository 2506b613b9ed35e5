"""kmws_gather_unmask_utf8 / kmws_unpack_gather_utf8 on the device: the gather's
output against kmws_gather_unmask and the plain payloads, the verdicts against
tests/utf8_ref.py, the carry against kmws_utf8_validate on the dense output --
every case in both copy forms (chunks below 16 KiB of dst_cap per frame, units
from it), chosen by dst_cap alone for the same batch."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import test_gpu_utf8 as vt
import utf8_ref as ref
from test_gpu_utf8 import B_, C_, FIN, PING, RSV1, T_, Batch

FILL = 0xAB
FORMS = ("chunk", "unit")
UNIT_FROM = 16384  # dst_cap / n from which the unit form runs


def both_forms(frames):
    """The frames, with empty PING frames appended until the mean payload is
    below the unit form's threshold: then dst_cap alone selects the form."""
    frames = list(frames)
    total = sum(len(p) for _, p in frames)
    while frames and ((total + 15) // 16 * 16 + 16) // len(frames) >= UNIT_FROM:
        frames.append((PING | FIN, b""))
    return frames


def dst_cap_of(form, n, total):
    tight = (total + 15) // 16 * 16 + 16
    cap = tight if form == "chunk" else max(UNIT_FROM * n, tight)
    if n:
        assert (cap // n < UNIT_FROM) == (form == "chunk"), (form, n, total)
    return cap


def run_gather(batch, form, stream_first=None, carry_in=None, lo=0, hi=None, cap=None):
    """Frames [lo, hi) of the batch through the fused call, the plain gather and
    kmws_utf8_validate on the plain gather's output; asserts (i), (iii) and (iv)
    of the module's contract and returns (verdicts, carry_out)."""
    import torch as T
    from kuma_amd import kmws
    hi = batch.n if hi is None else hi
    n = hi - lo
    lens = batch.lens[lo:hi]
    total = int(lens.sum())
    cap = dst_cap_of(form, n, total) if cap is None else cap
    src = T.from_numpy(batch.masked()).cuda()
    descs = kmws.make_descs(batch.offs[lo:hi], lens, batch.keys[lo:hi].astype(np.int64))
    fl = T.from_numpy(batch.flags[lo:hi].astype(np.int16)).cuda()
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
            ws = kmws.Workspace(kmws.gather_utf8_workspace_size(n, cap, ns))
            kmws.gather_unmask_utf8(src, descs, fl, dst, off, out, ws, stream_first=sf, carry_in=ci, carry_out=co)
        else:
            ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
            kmws.gather_unmask(src, descs, dst, off, ws)
        assert ws.status() == 0, (form, fused)
        if not fused and n:  # the validator on the dense output, descriptors from dst_off
            dd = kmws.make_descs(off[:n].cpu().numpy(), lens, np.zeros(n, dtype=np.int64))
            wv = kmws.Workspace(kmws.utf8_workspace_size(total, n, ns))
            kmws.utf8_validate(dst, dd, fl, out, wv, span=total, masked=False, stream_first=sf, carry_in=ci,
                               carry_out=co)
            assert wv.status() == 0
        res[fused] = (dst, off, out, co)
    assert T.equal(src, T.from_numpy(batch.masked()).cuda()), "src was written"
    (dst, off, out, co), (dst2, off2, out2, co2) = res[True], res[False]
    want_off = np.concatenate([[0], np.cumsum(lens)])
    assert np.array_equal(off.cpu().numpy(), want_off) and T.equal(off, off2), form
    plain = np.frombuffer(b"".join(p for _, p in batch.frames[lo:hi]), dtype=np.uint8)
    got = dst[:total].cpu().numpy()
    assert np.array_equal(got, plain), (form, np.nonzero(got != plain)[0][:8])
    assert T.equal(dst, dst2), form  # the plain gather's bytes, and the fill past the total
    assert bool((dst[total:] == FILL).all()), form
    if n:
        assert T.equal(co, co2), (form, co.cpu().numpy(), co2.cpu().numpy())
        assert T.equal(out[:n], out2[:n]), (form, T.nonzero(out[:n] != out2[:n])[:8])
    return out.cpu().numpy()[:n], co.cpu().numpy()[:ns]


def check(batch, expect=None, forms=FORMS, **kw):
    expect = vt.want(batch.frames) if expect is None else np.asarray(expect, dtype=np.uint8)
    for form in forms:
        out, _ = run_gather(batch, form, **kw)
        bad = np.nonzero(out != expect)[0]
        assert bad.size == 0, (form, bad[:10], out[bad[:10]], expect[bad[:10]])
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

# (unit of dst, how many of its multiples from the frame's first byte on): the 16-byte word, the
# 64-byte ownership granule, a wave-instruction's 1 KiB row (all four rows of a unit, twice), a
# 4 KiB unit / chunk
OUT_CLASSES = ((16, 4), (64, 4), (1024, 8), (4096, 4))


def out_sweep_copies(off):
    """Corruptions (class unit, p, new byte) of a copy at dst offset off, with
    off + p within +-4 bytes of a multiple of the unit."""
    _, arr = vt.sweep_text()
    seen, res = set(), []
    for unit, count in OUT_CLASSES:
        m0 = (off + unit - 1) // unit * unit
        for k in range(count):
            for dlt in range(-4, 5):
                p = m0 + k * unit + dlt - off
                if not 0 <= p < vt.SWEEP_LEN or p in seen:
                    continue
                seen.add(p)
                res.append((unit, p, 0xFF))
                width = 2 if 0xC2 <= arr[p] <= 0xDF else 3 if 0xE0 <= arr[p] <= 0xEF else 4 if arr[p] >= 0xF0 else 0
                if width and p + width <= vt.SWEEP_LEN:
                    res.append((unit, p + width - 1, 0x61))  # truncated: its last continuation becomes "a"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("r", range(16))
def test_boundary_sweep_in_output_space(r):
    data, _ = vt.sweep_text()
    assert vt.SWEEP_LEN % 4096 == 0  # every copy lies at r past a 4 KiB edge of dst: one list serves all
    plan = [None] + out_sweep_copies(r)
    frames = both_forms([(B_ | FIN, bytes(range(0x80, 0x80 + r)))] + [(T_ | FIN, data)] * len(plan))
    for s in (r, (r + 1) % 16, (r + 7) % 16, (r + 12) % 16):  # src offset mod 16: delta = 0 and three others
        offs, pos = [], 0
        for _, p in frames:
            pos = (pos + 15) // 16 * 16 + 16 + s
            offs.append(pos)
            pos += len(p)
        b = Batch(frames, offs, pos + 5, seed=r)
        expect, classes = [ref.NOT_TEXT], {}
        for j, c in enumerate(plan):
            off = offs[1 + j]
            assert off % 16 == s
            if c is None:
                expect.append(ref.OK)
                continue
            unit, p, newb = c
            b.plain[off + p] = newb
            b.frames[1 + j] = (T_ | FIN, bytes(b.plain[off:off + vt.SWEEP_LEN]))
            expect.append(vt.sweep_verdict(b.plain[off:off + vt.SWEEP_LEN], p))
            classes[unit] = classes.get(unit, 0) + 1
        expect += [ref.NOT_TEXT] * (len(frames) - len(expect))
        assert expect[1] == ref.OK and all(e == ref.BAD for e in expect[2:2 + len(plan) - 1])
        assert all(classes.get(u, 0) >= 1 for u, _ in OUT_CLASSES), classes
        check(b, expect)


# ---------------------------------------------------------------- 3. fragment straddles

@pytest.mark.gpu
def test_fragment_straddles():
    rng = random.Random(7)
    frames = vt.straddle_frames(rng)
    expect = vt.want(frames)
    assert set(expect) == {0, 1, 2, 3}
    assert any(b0 == (C_ | FIN) and p == b"" and e == ref.BAD for (b0, p), e in zip(frames, expect))
    assert any((b0 & 0x0F) == PING and p for b0, p in frames)
    check(packed(frames, 7), expect)


@pytest.mark.gpu
@pytest.mark.parametrize("top", [1, 3], ids=["dense_0_1", "frames_0_to_3"])
def test_tiny_fragments_across_scan_tiles(top):
    """n = 3 * 2048 + 7 frames of 0..top bytes: every code point straddles
    fragments, a 4 KiB chunk holds far more than 64 frames (chunk_dense_kernel),
    the chunk scan's look-back crosses its 2048-frame tiles and the UTF-8 scan
    its 256-frame blocks."""
    n = 3 * 2048 + 7
    lens = np.random.default_rng(50 + top).integers(0, top + 1, size=n)
    frames = vt.fill_messages(lens, 60 + top)
    assert 4096 // max(int(lens.sum()) // n, 1) > 64
    expect = vt.want(frames)
    assert {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD} <= set(expect)
    check(packed(frames, 51), expect)


# ---------------------------------------------------------------- 4. layouts

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tiny_many", "zero_len_runs", "packed_wire", "long_gaps"])
def test_layouts(kind):
    offs, lens, total = vt.layout(kind, np.random.default_rng(5))
    frames = vt.fill_messages(lens, 11)
    pad = both_forms(frames)[len(frames):]  # empty frames: anywhere in the arena
    b = Batch(frames + pad, list(offs) + [0] * len(pad), total)
    expect = check(b)
    assert {ref.NOT_TEXT, ref.OK, ref.BAD} <= set(expect)


@pytest.mark.gpu
def test_descriptors_in_descending_source_order():
    lens = np.random.default_rng(6).choice([0, 1, 5, 17, 300, 4096, 5000, 20000], size=60)
    frames = vt.fill_messages(lens, 12)
    offs, total = vt.packed_offsets([len(p) for _, p in frames][::-1], random.Random(6))
    offs = offs[::-1]  # frame i lies before frame i - 1 in src
    assert all(a > b for a, b in zip(offs, offs[1:]))
    b = Batch(frames, offs, total)
    expect = check(b)
    assert {ref.OK, ref.BAD} <= set(expect)


# ---------------------------------------------------------------- 5. streams and carry

@pytest.mark.gpu
def test_streams_in_one_call():
    b, first, expect = vt.stream_batch()
    check(b, expect, stream_first=first)


@pytest.mark.gpu
def test_streams_cut_into_two_calls_joined_by_the_carry():
    b, first, expect = vt.stream_batch()
    s5, s6, s8 = (int(first[s]) for s in (5, 6, 8))
    for c in (s5 + 1, s5 + 2, s6 + 1, s6 + 3, s8 + 1, int(first[21]), b.n // 2):
        f1 = np.minimum(first, c)
        f2 = np.maximum(first, c) - c
        for form in FORMS:
            out1, carry = run_gather(b, form, stream_first=f1, lo=0, hi=c)
            out2, _ = run_gather(b, form, stream_first=f2, carry_in=carry, lo=c)
            assert np.array_equal(out2, expect[c:]), (c, form, np.nonzero(out2 != expect[c:])[0][:10])
            assert np.array_equal(out1, expect[:c]), (c, form)


@pytest.mark.gpu
@pytest.mark.parametrize("second", [vt.OK_PIECE, vt.BAD_PIECE], ids=["ok", "bad"])
def test_message_open_across_rounds(second):
    """tests/test_gpu_utf8.py's round-two case through the fused gather: the frame
    state crosses the first round of the aggregate scan (run_gather checks the
    dense payload and the offsets as ever)."""
    frames, at = vt.round_edge_frames(*vt.EDGE_ROUNDS[2], second)
    expect = vt.round_edge_expect(frames, at, second)
    out, carry = run_gather(vt.round_edge_batch(frames), "chunk")
    bad = np.nonzero(out != expect)[0]
    assert bad.size == 0, (bad[:10], out[bad[:10]], expect[bad[:10]])
    assert bytes(carry[0]) == vt.scan_carry_after(frames, expect, bytes(8))


# ---------------------------------------------------------------- 6. unpack form

def run_unpack(wire, hdr, form, fused):
    import torch as T
    from kuma_amd import kmws
    W, n = len(wire), len(hdr)
    cap = dst_cap_of(form, n, W)
    w = T.zeros((W + 15) // 16 * 16, dtype=T.uint8, device="cuda")
    w[:W] = T.from_numpy(np.ascontiguousarray(wire)).cuda()
    d_hdr = T.tensor(hdr, dtype=T.int64, device="cuda")
    desc = T.zeros((n, 2), dtype=T.int64, device="cuda")
    fl = T.zeros(n, dtype=T.int16, device="cuda")
    err = T.full((n,), 99, dtype=T.uint8, device="cuda")
    out = T.full((n,), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((1, 8), 0xEE, dtype=T.uint8, device="cuda")
    dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
    off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    if fused:
        ws = kmws.Workspace(kmws.gather_utf8_workspace_size(n, cap, 1))
        kmws.unpack_gather_utf8(w, d_hdr, kmws.SERVER, desc, fl, err, dst, off, out, ws, wire_len=W, carry_out=co)
        status = ws.status()
    else:
        ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
        kmws.unpack_gather(w, d_hdr, kmws.SERVER, desc, fl, err, dst, off, ws, wire_len=W)
        status = ws.status()
        total = int(off[n].item())
        lens = (desc.cpu().numpy()[:, 1] & 0xFFFFFFFF).astype(np.int64)
        dd = kmws.make_descs(off[:n].cpu().numpy(), lens, np.zeros(n, dtype=np.int64))
        wv = kmws.Workspace(kmws.utf8_workspace_size(total, n, 1))
        kmws.utf8_validate(dst, dd, fl, out, wv, span=total, masked=False, carry_out=co)
        assert wv.status() == 0
    assert np.array_equal(w[:W].cpu().numpy(), wire), "the wire was written"
    return tuple(t.cpu().numpy() for t in (desc, fl, err, dst, off, out, co)) + (status,)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_unpack_gather_utf8_equals_the_two_calls(form):
    import test_gpu_unmask_utf8 as fu
    frames = fu.unpack_frames(80)
    ops = {(b0 & 0x0F, bool(b0 & RSV1)) for b0, _ in frames}
    assert {(T_, False), (B_, False), (T_, True)} <= ops and any(op >= 8 for op, _ in ops)
    wire, hdr = fu.server_wire(frames, 81)
    wire = wire.copy()
    heads = [i for i, (b0, p) in enumerate(frames) if (b0 & 0x4F) == T_ and len(p) > 200]
    bad = [heads[0], heads[-1]]
    for i in bad:
        wire[hdr[i] + 1] &= 0x7F  # no MASK bit: a server rejects the unmasked non-empty frame
    got = run_unpack(wire, hdr, form, True)
    two = run_unpack(wire, hdr, form, False)
    assert got[7] == 2 and two[7] == 2
    for name, a, b_ in zip(("out_desc", "out_flags", "out_err", "dst", "dst_off", "out_utf8", "carry_out"), got, two):
        assert np.array_equal(a, b_), (name, np.nonzero(np.asarray(a).reshape(-1) != np.asarray(b_).reshape(-1))[0][:8])
    assert all(got[2][i] == 7 for i in bad) and int((got[2] != 0).sum()) == 2
    # the reference on what the frames became: the two error frames are empty
    became = [(b0, b"" if i in bad else p) for i, (b0, p) in enumerate(frames)]
    assert np.array_equal(got[5], vt.want(became))
    total = int(got[4][-1])
    assert bytes(got[3][:total]) == b"".join(p for _, p in became)


# ---------------------------------------------------------------- 7. contract

def small_batch():
    frames = [(T_ | FIN, b"abc"), (T_ | FIN, "€".encode()), (T_ | FIN, b"\xff"), (T_ | FIN, b"z" * 40)]
    return Batch(frames, [4, 20, 40, 60], 128)


def raw_call(L, b, cap, stream_first=None, n=None, carry_in=None):
    """The C entry on its own buffers: (rc, status, dst, dst_off, carry_out)."""
    import torch as T
    from kuma_amd import kmws
    n = b.n if n is None else n
    src = T.from_numpy(b.masked()).cuda()
    descs = kmws.make_descs(b.offs, b.lens, b.keys.astype(np.int64))
    fl = T.from_numpy(b.flags.astype(np.int16)).cuda()
    ns = 1 if stream_first is None else len(stream_first) - 1
    sf = None if stream_first is None else T.tensor(list(stream_first), dtype=T.int32, device="cuda")
    ci = None if carry_in is None else T.from_numpy(np.ascontiguousarray(carry_in, dtype=np.uint8)).cuda()
    dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
    off = T.full((b.n + 1,), -1, dtype=T.int64, device="cuda")
    out = T.full((b.n,), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((ns, 8), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(L.kmws_gather_utf8_workspace_size(n, cap, ns))
    h = kmws._stream_handle()
    rc = L.kmws_gather_unmask_utf8(src.data_ptr(), descs.data_ptr(), fl.data_ptr(), n, dst.data_ptr(), cap,
                                   off.data_ptr(), kmws._opt(sf), ns, kmws._opt(ci), co.data_ptr(), out.data_ptr(),
                                   ws.ptr, ws.nbytes, h)
    st = C.c_uint32(0)
    assert L.kmws_read_status(ws.ptr, C.byref(st), h) == 0
    return rc, st.value, dst.cpu().numpy(), off.cpu().numpy(), co.cpu().numpy()


@pytest.mark.gpu
def test_contract_cap_streams_and_empty_batch():
    from kuma_amd import kmws
    L = kmws.lib()
    good = small_batch()
    total = int(good.lens.sum())
    assert list(check(good)) == [1, 1, 2, 1]
    # total > dst_cap: status bit 1, nothing stored -- the chunk form, then the unit form
    rc, st, dst, _, _ = raw_call(L, good, 32)
    assert rc == 0 and st & 1 and (dst == FILL).all()
    big = Batch([(T_ | FIN, b"q" * 20000)] * 3, [16, 20032, 40048], 60064)
    assert UNIT_FROM * 3 < 60000
    rc, st, dst, _, _ = raw_call(L, big, UNIT_FROM * 3)
    assert rc == 0 and st & 1 and (dst == FILL).all()
    for form in FORMS:
        cap = dst_cap_of(form, good.n, total)
        for sf in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3], [0, 5, 4]):
            rc, st, _, _, _ = raw_call(L, good, cap, stream_first=sf)
            assert rc == 0 and st & 1, (form, sf)
        rc, st, dst, off, _ = raw_call(L, good, cap, stream_first=[0, 0, 2, 2, 4, 4])
        assert rc == 0 and st == 0 and off[-1] == total
    # n == 0: OK, dst_off[0] = 0, carry_out = carry_in
    carry = np.arange(24, dtype=np.uint8).reshape(3, 8)
    rc, st, dst, off, co = raw_call(L, good, 64, stream_first=[0, 0, 0, 0], n=0, carry_in=carry)
    assert rc == 0 and st == 0 and off[0] == 0 and np.array_equal(co, carry) and (dst == FILL).all()
    out, co = run_gather(good, "chunk", lo=0, hi=0, cap=64)
    assert out.size == 0 and np.array_equal(co, np.zeros((1, 8), dtype=np.uint8))


@pytest.mark.gpu
def test_chunk_scan_lookback_timeout_sets_bit_4_and_stores_nothing():
    """The test-hooks build (one scan tile never publishes): the fused entry
    reports the look-back timeout as kmws_gather_unmask does -- status bit 4,
    not bit 1, nothing stored."""
    from kuma_amd import build as kb
    from kuma_amd import kmws
    assert os.path.exists(kb.TEST_LIB), "run __graft_entry__.build()"
    TL = kmws.bind(C.CDLL(kb.TEST_LIB))
    n = 3 * 2048 + 7
    lens = np.random.default_rng(45).integers(1, 120, size=n)
    frames = [(T_ | FIN, bytes([0x61 + i % 26]) * int(L)) for i, L in enumerate(lens)]
    b = Batch(frames, np.arange(n, dtype=np.int64) * 128, n * 128)
    cap = int(lens.sum()) + 16
    assert cap // n < UNIT_FROM  # the chunk form: chunk_scan_kernel's look-back
    rc, st, dst, _, _ = raw_call(TL, b, cap)
    assert rc == 0 and st & 4 and not st & 1, st
    assert (dst == FILL).all()
    rc, st, dst, off, _ = raw_call(kmws.lib(), b, cap)  # the product library on the same batch
    assert rc == 0 and st == 0 and off[-1] == lens.sum()


# ---------------------------------------------------------------- 8. captured graph

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
    total = int(b.lens.sum())
    cap = dst_cap_of(form, n, total)
    src = T.from_numpy(b.masked()).cuda()
    descs = kmws.make_descs(b.offs, b.lens, b.keys.astype(np.int64))
    fl = T.from_numpy(b.flags.astype(np.int16)).cuda()
    dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
    off = T.zeros(n + 1, dtype=T.int64, device="cuda")
    out = T.full((n,), 0xEE, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.gather_utf8_workspace_size(n, cap, 1))
    call = lambda: kmws.gather_unmask_utf8(src, descs, fl, dst, off, out, ws)
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
        assert int(dst[p].item()) == int(newb) and bytes(dst[50000:50004].cpu().numpy()) == b"tail"


# ---------------------------------------------------------------- 9. fuzz

def test_fuzz_mix_is_informative():
    """CPU, on the reference's verdicts over the batches test_fuzz runs: every
    verdict value occurs, and both valid and invalid checked messages, with an
    invalid one whose BAD frame is not its first."""
    seen, valid, invalid, late = set(), 0, 0, 0
    for k in range(vt.FUZZ_BATCHES):
        _, _, expect, streams, per_stream = vt.fuzz_batch(k)
        seen |= set(int(v) for v in expect)
        v, i, l = vt.fuzz_mix(streams, per_stream)
        assert v >= 1 and i >= 1, k
        valid, invalid, late = valid + v, invalid + i, late + l
    assert seen == {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD}
    assert valid * 4 >= valid + invalid and invalid * 4 >= valid + invalid and late >= vt.FUZZ_BATCHES


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(vt.FUZZ_BATCHES))
def test_fuzz(k):
    b, first, expect, _, _ = vt.fuzz_batch(k)
    pad = both_forms(b.frames)[b.n:]  # empty frames of the last stream
    if pad:
        first = np.concatenate([first[:-1], [first[-1] + len(pad)]])
        b = Batch(b.frames + pad, list(b.offs) + [0] * len(pad), b.total, seed=k)
        expect = np.concatenate([expect, np.full(len(pad), ref.NOT_TEXT, dtype=np.uint8)])
    check(b, expect, stream_first=first)
