"""kmws_unmask_utf8_batch / kmws_unpack_unmask_utf8 on the device: the fused
in-place unmask + UTF-8 validation against the two contracts it composes.  The
verdict reference is tests/utf8_ref.py (pinned by tests/test_utf8_ref.py); the
expected bytes are the plain payloads the test built (Batch.plain) or the
oracle's unmask.  Every case asserts the whole arena (gaps and rounding tail
included), the verdicts, and status 0 (unmask_utf8_util.check_fused)."""
import functools
import random

import numpy as np
import pytest

import unmask_utf8_util as u
import utf8_ref as ref
from oracle import oracle as orc

vt = u.vt
Batch, T_, C_, B_, FIN, RSV1, PING = u.Batch, u.T_, u.C_, u.B_, u.FIN, u.RSV1, u.PING

SCHEDULES = [k | s for k in range(6) for s in (0, 1 << 30)]  # every placement kind, default and temporal stores


# ---------------------------------------------------------------- 1. known answers

@pytest.mark.gpu
def test_known_answers():
    frames, expect = [], []
    for data, ok in vt.KNOWN:
        assert ref.valid(data) == ok
        frames += [(T_ | FIN, data), (B_ | FIN, data), (T_ | FIN | RSV1, data)]
        expect += [ref.OK if ok else ref.BAD, ref.NOT_TEXT, ref.NOT_TEXT]
    offs, total = vt.packed_offsets([len(p) for _, p in frames], random.Random(1))
    assert list(vt.want(frames)) == expect
    u.check_fused(Batch(frames, offs, total), expect)


# ---------------------------------------------------------------- 2. boundary sweep

@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["covered64k", "packed"])
@pytest.mark.parametrize("o", range(16))
def test_boundary_sweep(o, aligned):
    """One corruption within +-4 bytes of every 16 B / 1 KiB / 4 KiB / 16 KiB
    boundary of a 40 KiB text: every place where the look-back changes source
    (neighbour lane, row hand-over, saved tile edge), on covered tiles and on
    tiles of two frames."""
    b, expect, classes = u.sweep_batch(o, aligned)
    assert expect[0] == ref.OK and all(e == ref.BAD for e in expect[1:])
    assert all(classes.get(unit, 0) >= 1 for unit, _ in vt.SWEEP_CLASSES), classes
    u.check_fused(b, expect)


# ---------------------------------------------------------------- 3. valid text across every boundary

WIDE_BYTES = 8 * 1024 * 1024 // 12 * 12  # 8 MiB rounded down to whole 3- and 4-byte code points


def wide_batch(width, layout, o):
    data = u.wide_text(width, WIDE_BYTES, 300 + width)
    if layout == "fragments":  # one message, 64 KiB non-FIN fragments back to back from arena offset o
        cuts = list(range(0, WIDE_BYTES, 65536)) + [WIDE_BYTES]
        frames = [((T_ if i == 0 else C_), bytes(data[a:e])) for i, (a, e) in enumerate(zip(cuts, cuts[1:]))]
        offs = [a + o for a in cuts[:-1]]
        total = WIDE_BYTES + o
    else:                      # 128 FIN messages of whole code points, one per 64 KiB slot
        L = 65536 // width * width
        frames = [(T_ | FIN, bytes(data[i * L:(i + 1) * L])) for i in range(128)]
        offs = [i * 65536 for i in range(128)]
        total = 128 * 65536
    return u.nonzero_keys(Batch(frames, offs, total, seed=width))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["fragments", "messages"])
@pytest.mark.parametrize("width", [3, 4])
def test_valid_wide_text_across_every_boundary(width, layout):
    """8 MiB of 3-byte (4-byte) code points, so that nearly every 1 KiB row and
    16 KiB tile boundary splits one, unmasked and validated by 512 blocks at
    once under every schedule: every frame OK, every byte unmasked.

    What this cannot do: a look-back read from bytes that another wave or block
    may already have unmasked would fail only now and then, so a pass narrows
    the odds and proves nothing.  What rules the race out is the kernel's
    construction (kmws_utf8.hip, "the fused in-place pass"): no look-back is
    read from the payload while the pass runs -- the dword before a tile was
    saved ahead of it in stream order, the dword before a row comes from the
    registers of the wave that loaded it."""
    import torch as T
    from kuma_amd import kmws
    for o in ((0, 1, 2, 3) if layout == "fragments" else (0,)):
        b = wide_batch(width, layout, o)
        assert all(k != 0 for k in b.keys)
        expect = np.full(b.n, ref.OK, dtype=np.uint8)
        if o == 0:
            assert np.array_equal(vt.want(b.frames), expect)  # the reference agrees (once: it is slow on 8 MiB)
        dev = u.device_inputs(b)
        plain = T.from_numpy(b.plain).cuda()
        want = T.from_numpy(expect).cuda()
        out = T.empty(b.n, dtype=T.uint8, device="cuda")
        for sched in SCHEDULES:
            base = dev["masked"].clone()
            out.fill_(0xEE)
            kmws.unmask_utf8(base, dev["descs"], dev["fl"], out, dev["ws"], span=b.total, schedule=sched)
            assert T.equal(out, want), (o, sched, T.nonzero(out != want)[:10].flatten().tolist())
            assert T.equal(base, plain), (o, sched)
            assert dev["ws"].status() == 0


# ---------------------------------------------------------------- 4. general path

@functools.lru_cache(maxsize=None)
def batch_700_frames():
    """The batch, its frames and the reference's verdicts: built once for every schedule."""
    rng = random.Random(70)
    lens = [rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 21, 34, 40]) for _ in range(700)]
    frames = vt.fill_messages(lens, 71) + vt.straddle_frames(rng)
    offs, pos = [], 0
    for _, p in frames:
        pos += rng.randint(0, 3)
        offs.append(pos)
        pos += len(p)
    assert len(frames) > 700 and offs[699] + len(frames[699][1]) <= 16384  # 700 frames inside the first tile
    b = Batch(frames, offs, pos + 5)
    return b, frames, vt.want(b.frames)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", SCHEDULES)
def test_general_path_700_frames_in_one_tile(sched):
    """More than two LDS rounds of descriptors in one tile: text fragments with
    code points straddling frames, PINGs, binary and RSV1 messages, empty FIN
    frames that end inside a code point, key-0 and len-0 frames.  Under every
    schedule, and the arena also equals what kmws_unmask_batch leaves on a fresh
    masked copy: the plain apply's second and third rounds of the same staged
    masks."""
    import torch as T
    from kuma_amd import kmws
    b, frames, expect = batch_700_frames()
    u.check_fused(b, expect, schedule=sched)
    assert {ref.NOT_TEXT, ref.OK, ref.BAD, ref.AFTER_BAD} <= set(expect)
    assert any(k == 0 for k in b.keys) and any(L == 0 for L in b.lens)
    empties = [i for i, (b0, p) in enumerate(frames) if b0 == (C_ | FIN) and p == b""]
    assert {int(expect[i]) for i in empties} >= {ref.OK, ref.BAD}
    assert any((b0 & 0x0F) == PING for b0, _ in frames)
    plain = T.from_numpy(b.masked()).cuda()
    ws = kmws.Workspace(kmws.unmask_workspace_size(b.total))
    kmws.unmask_batch(plain, kmws.make_descs(b.offs, b.lens, b.keys.astype(np.int64)), ws, b.total)
    assert ws.status() == 0
    assert np.array_equal(plain.cpu().numpy(), u.expected_arena(b))


@pytest.mark.gpu
def test_general_path_4k_fragments():
    lens = [4096] * 64
    frames = vt.fill_messages(lens, 72)
    offs, total = vt.packed_offsets(lens, random.Random(73))
    expect, _ = u.check_fused(Batch(frames, offs, total))
    assert {ref.NOT_TEXT, ref.OK, ref.BAD} <= set(expect)


# ---------------------------------------------------------------- 5. span edges

SPAN_EDGE_CASES = ["below_one_tile", "three_tiles_and_a_byte", "ends_on_the_last_byte"]


@functools.lru_cache(maxsize=None)
def span_edge_batch(case):
    """The batch and the reference's verdicts: built once for every schedule."""
    pool = ref.TextPool(random.Random(50), size=1 << 16)
    rng = random.Random(51)
    if case == "below_one_tile":      # 5 KiB: the tail kernel alone
        lens = [700, 0, 1500, 33, 2000]
        offs, _ = vt.packed_offsets(lens, rng)
        total = 5 * 1024
    elif case == "three_tiles_and_a_byte":  # the split grid, and a tail tile of one byte, the last frame's last
        total = 3 * 16384 + 1
        offs = [5, 20010, 20020]
        lens = [20000, 3, total - 20020]
    else:                              # the last frame's last byte is the span's, mid-tile
        lens = [16384, 16384 + 777]
        offs = [9, 16400]
        total = offs[1] + lens[1]
    frames = [(T_ | FIN, pool.take(rng, L)) for L in lens]
    if case != "below_one_tile":       # the message ends inside a code point, on the span's last byte
        frames[-1] = (T_ | FIN, frames[-1][1][:-1] + b"\xe2")
    b = Batch(frames, offs, total)
    return b, vt.want(b.frames)


@pytest.mark.gpu
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("case", SPAN_EDGE_CASES)
def test_span_edges(case, sched):
    """three_tiles_and_a_byte: the two-frame path, the split grid and the tail
    kernel together, under every schedule."""
    b, expect = span_edge_batch(case)
    assert b.offs[-1] + b.lens[-1] <= b.total
    if case != "below_one_tile":
        assert b.offs[-1] + b.lens[-1] == b.total
    u.check_fused(b, expect, schedule=sched)
    assert expect[-1] == (ref.OK if case == "below_one_tile" else ref.BAD) and ref.OK in expect


# ---------------------------------------------------------------- 6. streams and carry

@pytest.mark.gpu
def test_streams_in_one_call_and_the_validators_carry():
    b, first, expect = vt.stream_batch()
    _, carry = u.check_fused(b, expect, stream_first=first)
    assert {0, 1, 2, 3} <= set(expect)
    _, carry_v, st = vt.run_gpu(b, masked=True, stream_first=first)
    assert st == 0 and np.array_equal(carry, carry_v)


@pytest.mark.gpu
def test_streams_cut_into_two_calls_joined_by_the_carry():
    b, first, expect = vt.stream_batch()
    rng = random.Random(38)
    s5, s6, s7, s8 = (int(first[s]) for s in (5, 6, 7, 8))
    cuts = {s5 + 1, s5 + 2, s6 + 1, s6 + 2, s6 + 3, s7 + 1, s7 + 2, s8 + 1, int(first[3]), int(first[21])}
    cuts |= {rng.randrange(1, b.n) for _ in range(6)}
    after_bad_through_carry = 0
    for c in sorted(cuts):
        f1 = np.minimum(first, c)
        f2 = np.maximum(first, c) - c
        a1, out1, carry1, st1 = u.run_fused(b, stream_first=f1, lo=0, hi=c)
        a2, out2, carry2, st2 = u.run_fused(b, stream_first=f2, carry_in=carry1, lo=c)
        assert st1 == 0 and st2 == 0
        assert np.array_equal(a1, u.expected_arena(b, 0, c)) and np.array_equal(a2, u.expected_arena(b, c, b.n)), c
        got = np.concatenate([out1, out2])
        assert np.array_equal(got, expect), (c, np.nonzero(got != expect)[0][:10])
        after_bad_through_carry += int(c < b.n and expect[c] == ref.AFTER_BAD)
        # byte-equal to what the validator writes for the same two batches
        _, cv1, sv1 = vt.run_gpu(b, masked=True, stream_first=f1, lo=0, hi=c)
        _, cv2, sv2 = vt.run_gpu(b, masked=True, stream_first=f2, carry_in=cv1, lo=c)
        assert sv1 == 0 and sv2 == 0
        assert np.array_equal(carry1, cv1) and np.array_equal(carry2, cv2), c
    assert after_bad_through_carry >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("second", [vt.OK_PIECE, vt.BAD_PIECE], ids=["ok", "bad"])
def test_message_open_across_rounds(second):
    """tests/test_gpu_utf8.py's round-two case through the fused entry: the frame
    state crosses the first round of the aggregate scan; the arena comes out plain."""
    frames, at = vt.round_edge_frames(*vt.EDGE_ROUNDS[2], second)
    expect = vt.round_edge_expect(frames, at, second)
    _, carry = u.check_fused(u.nonzero_keys(vt.round_edge_batch(frames)), expect)
    assert bytes(carry[0]) == vt.scan_carry_after(frames, expect, bytes(8))


# ---------------------------------------------------------------- 7. composition parity

FUZZ_SEEDS = range(40)


def test_fuzz_mix_on_the_reference():
    """CPU: over the 40 batches at least 20 % of the checked messages are BAD,
    at least 20 % OK, and at least 10 % of the frames NOT_TEXT -- on the
    reference's verdicts alone."""
    ok = bad = nt = frames = 0
    for k in FUZZ_SEEDS:
        _, _, _, streams, per_stream = vt.fuzz_batch(k)
        a, b_, c, d = u.mix_counts(streams, per_stream)
        ok, bad, nt, frames = ok + a, bad + b_, nt + c, frames + d
    assert ok + bad >= 400 and bad * 5 >= ok + bad and ok * 5 >= ok + bad and nt * 10 >= frames, (ok, bad, nt, frames)


@pytest.mark.gpu
def test_fuzz_composition_parity():
    """The arena equals kmws_unmask_batch's, out / carry_out equal
    kmws_utf8_validate(masked)'s on a fresh masked copy, and the reference's."""
    import torch as T
    from kuma_amd import kmws
    for k in FUZZ_SEEDS:
        b, first, expect, _, _ = vt.fuzz_batch(k)
        arena, out, carry, st = u.run_fused(b, stream_first=first)
        assert st == 0
        two = T.from_numpy(b.masked()).cuda()
        descs = kmws.make_descs(b.offs, b.lens, b.keys.astype(np.int64))
        kmws.unmask_batch(two, descs, kmws.Workspace(kmws.unmask_workspace_size(b.total)), b.total)
        out_v, carry_v, st_v = vt.run_gpu(b, masked=True, stream_first=first)
        assert st_v == 0
        assert np.array_equal(arena, two.cpu().numpy()), k
        assert np.array_equal(arena, b.plain), k
        assert np.array_equal(out, out_v) and np.array_equal(carry, carry_v), k
        bad = np.nonzero(out != expect)[0]
        assert bad.size == 0, (k, bad[:10], out[bad[:10]], expect[bad[:10]])


# ---------------------------------------------------------------- 8. kmws_unpack_unmask_utf8

def server_wire(frames, seed):
    """The frames (header byte 0, plain payload) as a client would send them:
    the oracle's encoder, every frame masked."""
    rng = np.random.default_rng(seed)
    lens = np.array([len(p) for _, p in frames], dtype=np.uint32)
    src = np.frombuffer(b"".join(p for _, p in frames) + b"\0", dtype=np.uint8).copy()
    src_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    flags = np.array([b0 | 0x100 for b0, _ in frames], dtype=np.uint32)
    keys = rng.integers(1, 2**32, size=len(frames), dtype=np.uint64).astype(np.uint32)
    wire, wire_off = orc.encode_batch(src, src_off, lens, flags, keys)
    return wire, wire_off.astype(np.int64)


def run_unpack(wire, hdr, fused, stream_first=None):
    """The fused entry, or kmws_unpack_unmask + kmws_utf8_validate on what it wrote."""
    import torch as T
    from kuma_amd import kmws
    W, n = len(wire), len(hdr)
    w = T.zeros((W + 15) // 16 * 16, dtype=T.uint8, device="cuda")
    w[:W] = T.from_numpy(np.ascontiguousarray(wire)).cuda()
    d_hdr = T.tensor(hdr, dtype=T.int64, device="cuda")
    desc = T.zeros((n, 2), dtype=T.int64, device="cuda")
    fl = T.zeros(n, dtype=T.int16, device="cuda")
    err = T.full((n,), 99, dtype=T.uint8, device="cuda")
    out = T.full((n,), 0xEE, dtype=T.uint8, device="cuda")
    ns = 1 if stream_first is None else len(stream_first) - 1
    sf = None if stream_first is None else T.tensor(list(stream_first), dtype=T.int32, device="cuda")
    co = T.full((ns, 8), 0xEE, dtype=T.uint8, device="cuda")
    if fused:
        ws = kmws.Workspace(kmws.unmask_utf8_workspace_size(W, n, ns))
        kmws.unpack_unmask_utf8(w, d_hdr, kmws.SERVER, desc, fl, err, out, ws, wire_len=W, stream_first=sf,
                                carry_out=co)
        status = ws.status()
    else:
        ws = kmws.Workspace(kmws.unmask_workspace_size(W))
        kmws.unpack_unmask(w, d_hdr, kmws.SERVER, desc, fl, err, ws, wire_len=W)
        status = ws.status()
        if not status & 1:
            wv = kmws.Workspace(kmws.utf8_workspace_size(W, n, ns))
            kmws.utf8_validate(w, desc, fl, out, wv, span=W, masked=False, stream_first=sf, carry_out=co)
            assert wv.status() == 0
    return tuple(t.cpu().numpy() for t in (w, desc, fl, err, out, co)) + (status,)


def unpack_frames(seed):
    rng = random.Random(seed)
    frames = vt.fill_messages([rng.choice([0, 1, 5, 125, 126, 300, 4096, 20000, 66000]) for _ in range(90)], seed)
    frames += vt.straddle_frames(rng)
    # a control frame carries at most 125 bytes (longer ones are header errors, which have their own test)
    return [(b0, p[:125] if (b0 & 0x0F) >= 8 else p) for b0, p in frames]


@pytest.mark.gpu
@pytest.mark.parametrize("streams", [False, True], ids=["one_stream", "streams"])
def test_unpack_unmask_utf8_equals_the_two_calls(streams):
    frames = unpack_frames(80)
    first = None
    expect = vt.want(frames)
    if streams:  # cut where no message is open, so that the reference can judge each stream alone
        closed = [i + 1 for i, (b0, _) in enumerate(frames) if (b0 & FIN) and (b0 & 0x0F) < 8]
        first = [0] + closed[3::7][:11] + [len(frames)]
        first = sorted(set(first)) + [len(frames)] * 2  # and two empty streams at the end
        expect = np.concatenate([np.array(ref.validate_stream(frames[a:e])[0], dtype=np.uint8)
                                 for a, e in zip(first, first[1:]) if e > a])
    wire, hdr = server_wire(frames, 81)
    got = run_unpack(wire, hdr, True, first)
    two = run_unpack(wire, hdr, False, first)
    assert got[6] == 0 and two[6] == 0
    for name, a, b_ in zip(("wire", "out_desc", "out_flags", "out_err", "out_utf8", "carry_out"), got, two):
        assert np.array_equal(a, b_), name
    assert not got[3].any()
    assert np.array_equal(got[4], expect) and {0, 1, 2, 3} <= set(expect)
    dd = got[1].view(orc.DESC_DTYPE).reshape(-1)
    assert b"".join(bytes(got[0][int(o):int(o) + int(L)]) for o, L in zip(dd["off"], dd["len"])) == \
        b"".join(p for _, p in frames)


@pytest.mark.gpu
def test_unpack_unmask_utf8_header_error_and_bad_offsets():
    """A header error: status bit 2, that frame empty and judged as such, the
    rest as kmws_unpack_unmask + kmws_utf8_validate; offsets out of order:
    status bit 1 and the wire unchanged."""
    frames = unpack_frames(82)
    wire, hdr = server_wire(frames, 83)
    wire = wire.copy()
    bad = next(i for i, (b0, p) in enumerate(frames) if (b0 & 0x4F) == T_ and len(p) > 200)  # a text head
    wire[hdr[bad] + 1] &= 0x7F  # no MASK bit: a server rejects the unmasked non-empty frame
    got = run_unpack(wire, hdr, True)
    two = run_unpack(wire, hdr, False)
    assert got[6] == 2 and two[6] == 2 and got[3][bad] == 7
    for name, a, b_ in zip(("wire", "out_desc", "out_flags", "out_err", "out_utf8", "carry_out"), got, two):
        assert np.array_equal(a, b_), name
    assert got[1].view(orc.DESC_DTYPE).reshape(-1)["len"][bad] == 0 and got[4][bad] == ref.OK
    swapped = hdr.copy()
    swapped[3], swapped[4] = hdr[4], hdr[3]
    w, _, _, _, _, _, status = run_unpack(wire, swapped, True)
    assert status & 1 and np.array_equal(w[:len(wire)], wire)


# ---------------------------------------------------------------- 9. contract

@pytest.mark.gpu
def test_contract_bad_descriptors_streams_and_empty_batch():
    frames = [(T_ | FIN, b"abc"), (T_ | FIN, "€".encode()), (T_ | FIN, b"\xff"), (T_ | FIN, b"z" * 40)]
    good = u.nonzero_keys(Batch(frames, [4, 20, 40, 60], 128))
    u.check_fused(good, [1, 1, 2, 1])

    from kuma_amd import kmws

    def untouched(dev=None, **kw):
        arena, _, _, st = u.run_fused(good, dev=dev, **kw)
        assert st & 1, kw
        assert np.array_equal(arena, good.masked()), kw

    for offs in ([4, 40, 20, 60], [4, 5, 40, 60], [4, 20, 40, 100]):  # unsorted, overlapping, past the span
        dev = u.device_inputs(good)
        dev["descs"] = kmws.make_descs(np.array(offs), good.lens, good.keys.astype(np.int64))
        untouched(dev)
    for sf in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 3], [0, 5, 4]):
        untouched(stream_first=sf)
    u.check_fused(good, [1, 1, 2, 1], stream_first=[0, 0, 2, 2, 4, 4])
    # n == 0: OK, carry_out = carry_in, nothing written
    carry = np.arange(24, dtype=np.uint8).reshape(3, 8)
    arena, out, co, _ = u.run_fused(good, stream_first=[0, 0, 0, 0], carry_in=carry, lo=0, hi=0)
    assert out.size == 0 and np.array_equal(co, carry) and np.array_equal(arena, good.masked())
    _, _, co, _ = u.run_fused(good, lo=0, hi=0)
    assert np.array_equal(co, np.zeros((1, 8), dtype=np.uint8))


@pytest.mark.gpu
def test_captured_graph_replays_on_a_remasked_arena():
    """The call holds kernel nodes only, enqueued on one stream: the capture is
    a single chain with no parallel branches.  Replayed on the arena masked
    again, with one byte corrupted, it unmasks and judges what is there now."""
    import torch as T
    from kuma_amd import kmws
    data = ref.text(random.Random(9), 50000)
    b = u.nonzero_keys(Batch([(T_ | FIN, data), (T_ | FIN, b"tail")], [6, 50020], 50040))
    dev = u.device_inputs(b)
    base = dev["masked"].clone()
    out = T.full((2,), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((1, 8), 0xEE, dtype=T.uint8, device="cuda")
    call = lambda: kmws.unmask_utf8(base, dev["descs"], dev["fl"], out, dev["ws"], span=b.total, carry_out=co)
    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(s):
        call()  # warm: every kernel loaded before the capture
    T.cuda.current_stream().wait_stream(s)
    T.cuda.synchronize()
    assert dev["ws"].status() == 0 and list(out.cpu().numpy()) == [1, 1]
    assert np.array_equal(base.cpu().numpy(), b.plain)
    g = T.cuda.CUDAGraph()
    base.copy_(dev["masked"])
    with T.cuda.graph(g):
        call()
    T.cuda.synchronize()
    p = 6 + 33333
    kb = int(b.keys[0]) >> (8 * (33333 & 3)) & 0xFF
    for newb, verdict in ((0xFF, 2), (int(b.plain[p]), 1)):
        base.copy_(dev["masked"])
        base[p] = newb ^ kb  # the masked form of the byte the message should hold
        out.fill_(0xEE)
        g.replay()
        T.cuda.synchronize()
        assert dev["ws"].status() == 0
        assert list(out.cpu().numpy()) == [verdict, 1]
        want = b.plain.copy()
        want[p] = newb
        assert np.array_equal(base.cpu().numpy(), want)
