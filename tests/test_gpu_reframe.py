"""kmws_reframe_batch / kmws_unpack_reframe against the oracle, byte for byte.

The expected bytes never come from kmws: every frame's source slice is unmasked
by the oracle with its incoming key (on a dense copy, so overlapping payloads
are fine), the skipped frames are dropped, and the oracle's encode_batch writes
the outgoing wire with flags & 0x1FF and the outgoing keys; wire_off of a
skipped frame repeats its predecessor's end.  For the fused entry the incoming
wire is built from raw headers (tests/header_cases.py) and the expected
out_desc / out_flags / out_err come from the oracle's decoder (hc.Expected).

Every run checks the workspace status, all of wire_off, dst[:total], and that
dst past the total and a 64-byte guard on each side of dst still hold the fill.
The copy form is chosen through dst_cap alone (cap // n < 16384: chunks).

The skips are the zero-byte regions the encode form never had: a frame flagged
KMWS_FLAG_SKIP has p0 == r0 == r1 in the copy kernels."""
import functools
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import header_cases as hc  # noqa: E402
import pack_edge_cases as pec  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xEE
GUARD = 64
FORMS = ("chunks", "units")
SKIP, MASK = 0x8000, 0x100
KINDS = ("as_built", "unmasked", "masked")  # the outgoing mask bits: the batch's own (mixed where it mixes), none, all


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


# ------------------------------ the reference ------------------------------
def reference(src, offs, lens, in_keys, flags, out_keys):
    """(wire, wire_off[n + 1]) from the oracle: unmask each kept frame's slice
    with its incoming key, encode with the outgoing flags and keys."""
    n = len(lens)
    flags = np.asarray(flags, dtype=np.uint32)
    keep = np.flatnonzero((flags & SKIP) == 0)
    sizes = np.zeros(n, dtype=np.int64)
    wire = np.zeros(0, dtype=np.uint8)
    if len(keep):
        kl = np.asarray(lens, dtype=np.int64)[keep]
        doff = np.concatenate([[0], np.cumsum(kl)[:-1]]).astype(np.uint64)
        dense = np.concatenate([src[int(offs[f]):int(offs[f]) + int(lens[f])] for f in keep] + [np.zeros(16, np.uint8)])
        d = np.zeros(len(keep), dtype=orc.DESC_DTYPE)
        d["off"], d["len"], d["key"] = doff, kl, np.asarray(in_keys, dtype=np.uint32)[keep]
        orc.unmask_batch(dense, d)
        ok = np.zeros(n, dtype=np.uint32) if out_keys is None else np.asarray(out_keys, dtype=np.uint32)
        ok = np.where(flags & MASK, ok, 0).astype(np.uint32)
        wire, woff = orc.encode_batch(dense, doff, kl, flags[keep] & 0x1FF, ok[keep])
        sizes[keep] = np.diff(np.concatenate([woff.astype(np.int64), [len(wire)]]))
    return wire, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def to_dev(T, a):
    pad = (-len(a)) % 16
    return T.from_numpy(np.concatenate([a, np.zeros(pad + 16, a.dtype)])).cuda()


def cap_for(form, n, total):
    cap = total + 5000 if form == "chunks" else max(total, pec.kChunkFormBelow * n) + 777
    assert (cap // n < pec.kChunkFormBelow) == (form == "chunks"), (form, n, cap)
    assert cap <= 80 << 20
    return cap


def guarded(T, cap):
    """dst of cap bytes inside a filled buffer with GUARD bytes on each side."""
    buf = T.full((GUARD + cap + GUARD,), FILL, dtype=T.uint8, device="cuda")
    return buf, buf[GUARD:GUARD + cap]


def first_true(mask):
    idx = mask.nonzero()
    return int(idx[0]) if idx.numel() else None


def check_output(T, tag, buf, dst, off, ws, want, want_off, status=0):
    T.cuda.synchronize()
    total = len(want)
    assert ws.status() == status, tag
    assert T.equal(off, T.from_numpy(want_off).cuda()), tag + ("first wrong offset",
                                                               first_true(off.cpu() != T.from_numpy(want_off)))
    d_want = T.from_numpy(np.ascontiguousarray(want)).cuda()
    assert T.equal(dst[:total], d_want), tag + ("first wrong byte", first_true(dst[:total] != d_want))
    assert bool((dst[total:] == FILL).all()), tag + ("first byte past the total", first_true(dst[total:] != FILL))
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + len(dst):] == FILL).all()), tag


def run_reframe(T, src, offs, lens, in_keys, flags, out_keys, forms=FORMS, d_src=None, tag=()):
    """One batch through kmws_reframe_batch in each form against the reference."""
    from kuma_amd import kmws
    n = len(lens)
    want, want_off = reference(src, offs, lens, in_keys, flags, out_keys)
    d_src = to_dev(T, src) if d_src is None else d_src
    descs = kmws.make_descs(np.asarray(offs).astype(np.int64), np.asarray(lens).astype(np.int64),
                            np.asarray(in_keys).astype(np.int64))
    d_fl = T.from_numpy(np.asarray(flags).astype(np.uint16).view(np.int16)).cuda()
    d_ok = None if out_keys is None else T.from_numpy(np.asarray(out_keys, dtype=np.uint32).view(np.int32)).cuda()
    for form in forms:
        cap = cap_for(form, n, len(want))
        buf, dst = guarded(T, cap)
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.reframe_batch(d_src, descs, d_fl, d_ok, dst, off, ws)
        check_output(T, tag + (form, n, len(want)), buf, dst, off, ws, want, want_off)
    return want, want_off


def mask_source(name, batch):
    """The batch's plain source masked per payload with random nonzero incoming
    keys (the payloads of pack_edge_cases batches do not overlap)."""
    src, offs, lens, flags, keys = batch
    rng = np.random.default_rng(zlib.crc32(("in-" + name).encode()))
    in_keys = rng.integers(1, 2**32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    d = np.zeros(len(lens), dtype=orc.DESC_DTYPE)
    d["off"], d["len"], d["key"] = offs, lens, in_keys
    masked = src.copy()
    orc.unmask_batch(masked, d)
    out_keys = rng.integers(1, 2**32, size=len(lens), dtype=np.uint64).astype(np.uint32)
    return masked, np.asarray(offs), np.asarray(lens), in_keys, np.asarray(flags, dtype=np.uint32), out_keys


def kind_flags(flags, kind):
    return {"as_built": flags, "unmasked": flags & ~np.uint32(MASK), "masked": flags | np.uint32(MASK)}[kind]


def run_edges(T, name, batch):
    src, offs, lens, in_keys, flags, out_keys = mask_source(name, batch)
    d_src = to_dev(T, src)
    for kind in KINDS:
        want, _ = run_reframe(T, src, offs, lens, in_keys, kind_flags(flags, kind), out_keys, d_src=d_src,
                              tag=(name, kind))
        if kind == "as_built":  # the plain source, encoded: the geometry the case was built for
            plain, _ = orc.encode_batch(batch[0], offs, lens, flags, np.where(flags & MASK, out_keys, 0))
            assert np.array_equal(want, plain)


# ------------------------------ edge geometry ------------------------------
@pytest.mark.parametrize("name", [k for k, c in pec.CASES.items() if c.encode])
def test_reframe_edge_cases(T, name):
    run_edges(T, name, pec.CASES[name].build(True))


@pytest.mark.parametrize("n", pec.COUNT_EDGES)
def test_reframe_frame_count_edges(T, n):
    run_edges(T, f"count-{n}", pec.frame_count_batch(n, True))


@pytest.mark.parametrize("out_phase", range(16))
def test_reframe_every_output_phase(T, out_phase):
    run_edges(T, f"phase-{out_phase}", pec.phase_batch(out_phase, True, mixed_masks=True))


# ------------------------------ key algebra ------------------------------
def test_reframe_key_algebra(T):
    from kuma_amd import kmws
    batch = pec.phase_batch(5, True, mixed_masks=True)
    plain_src, offs, lens, flags, keys = batch
    src, offs, lens, in_keys, flags, out_keys = mask_source("algebra", batch)
    n = len(lens)
    zero = np.zeros(n, dtype=np.uint32)
    # incoming key 0: the oracle's plain encode, and kmws_encode_batch's own output
    want, want_off = run_reframe(T, plain_src, offs, lens, zero, flags, out_keys, tag=("in0",))
    enc, enc_off = orc.encode_batch(plain_src, offs, lens, flags, np.where(flags & MASK, out_keys, 0))
    assert np.array_equal(want, enc) and np.array_equal(want_off[:n], enc_off.astype(np.int64))
    for form in FORMS:
        cap = cap_for(form, n, len(enc))
        dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
        off = T.zeros(n + 1, dtype=T.int64, device="cuda")
        ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
        ek = np.where(flags & MASK, out_keys, 0)
        kmws.encode_batch(to_dev(T, plain_src), kmws.make_descs(offs.astype(np.int64), lens, ek.astype(np.int64)),
                          T.from_numpy(flags.astype(np.int16)).cuda(), dst, off, ws, check=True)
        assert T.equal(dst[:len(enc)], T.from_numpy(enc).cuda())
    # incoming key == outgoing key, every frame masked: the payload is copied unchanged, the header carries the key
    allm = flags | np.uint32(MASK)
    want, want_off = run_reframe(T, src, offs, lens, in_keys, allm, in_keys, tag=("same",))
    for f in (0, 1, n // 2, n - 1):
        hl = int(pec.header_len(int(lens[f]), 1))
        a = int(want_off[f])
        assert bytes(want[a + hl:a + hl + int(lens[f])]) == bytes(src[int(offs[f]):int(offs[f]) + int(lens[f])])
        assert bytes(want[a + hl - 4:a + hl]) == int(in_keys[f]).to_bytes(4, "little")
    # keys whose XOR has zero bytes (0x11223344 ^ 0x11AA3344 = 0x00880000), and a zero XOR beside a nonzero one
    a_key, b_key = np.uint32(0x11223344), np.uint32(0x11AA3344)
    ik = np.where(np.arange(n) % 3 == 0, a_key, in_keys).astype(np.uint32)
    okk = np.where(np.arange(n) % 3 == 0, b_key, np.where(np.arange(n) % 3 == 1, ik, out_keys)).astype(np.uint32)
    d = np.zeros(n, dtype=orc.DESC_DTYPE)
    d["off"], d["len"], d["key"] = offs, lens, ik
    src2 = plain_src.copy()
    orc.unmask_batch(src2, d)
    run_reframe(T, src2, offs, lens, ik, allm, okk, tag=("zero-bytes",))
    # out_keys NULL with MASK set: every outgoing key is 0
    run_reframe(T, src, offs, lens, in_keys, allm, None, tag=("null-keys",))
    run_reframe(T, src, offs, lens, in_keys, flags, None, tag=("null-keys-mixed",))


# ------------------------------ skips ------------------------------
CHUNK = 4096


def fragment_batch():
    """2304 masked fragments whose outgoing frames are exactly 4 KiB (8 + 4088), so every frame starts a chunk; a
    few other lengths near the end."""
    n = 2304
    lens = np.full(n, 4088, dtype=np.int64)
    lens[-40:] = np.resize(np.array([0, 1, 125, 126, 300, 4096, 4097], dtype=np.int64), 40)
    flags = np.full(n, pec.FIN_BINARY | MASK, dtype=np.uint32)
    src, offs, keys = pec.layout_source("reframe-fragments", lens)
    return src, offs, lens, flags, keys


def region_sizes(lens, flags):
    live = (flags & SKIP) == 0
    return np.where(live, pec.header_len(lens, (flags >> 8) & 1) + lens, 0).astype(np.int64)


def align_frame_start(lens, flags, i):
    """Shortens live frames before frame i (shorter reads of the same source, the header class kept) until frame i
    starts on a 4 KiB output boundary."""
    r0 = np.concatenate([[0], np.cumsum(region_sizes(lens, flags))])
    left = int(r0[i]) % CHUNK
    for j in range(i - 1, -1, -1):
        if left == 0:
            break
        if not flags[j] & SKIP and 126 < lens[j] <= 0xFFFF:
            s = min(left, int(lens[j]) - 126)
            lens[j] -= s
            left -= s
    assert left == 0 and np.concatenate([[0], np.cumsum(region_sizes(lens, flags))])[i] % CHUNK == 0


SKIP_PATTERNS = ("every_third", "run65_on_chunk_boundary", "run_straddles_boundary", "whole_scan_tile", "last_frames",
                 "first_frame", "all", "wild_descriptors")


def skip_pattern(pattern, lens, flags):
    """(lens, flags) of one skip pattern over a batch (copies)."""
    n = len(lens)
    L, F = lens.copy(), flags.copy()
    if pattern == "every_third":
        F[::3] |= SKIP
    elif pattern == "run65_on_chunk_boundary":
        F[n // 3:n // 3 + 70] |= SKIP
        align_frame_start(L, F, n // 3)
    elif pattern == "run_straddles_boundary":
        # skipped frames on both sides of a boundary: 40 of them, one live frame longer than a chunk, 40 more
        mid = 2 * n // 3
        F[mid - 40:mid + 41] |= SKIP
        L[mid], F[mid] = 4096, pec.FIN_BINARY | MASK
    elif pattern == "whole_scan_tile":
        F[2048:4096] |= SKIP
        if n < 4096:
            F[:], F[:2048] = flags, flags[:2048] | SKIP
    elif pattern == "last_frames":
        F[n - 77:] |= SKIP
    elif pattern == "first_frame":
        F[0] |= SKIP
    elif pattern == "all":
        F[:] |= SKIP
    else:
        F[1::4] |= SKIP
    return L, F


@functools.lru_cache(maxsize=None)
def skip_batch(which):
    if which == "count":
        return mask_source("skip-count", pec.frame_count_batch(4097, True))
    return mask_source("skip-fragments", fragment_batch())


@pytest.mark.parametrize("pattern", SKIP_PATTERNS)
@pytest.mark.parametrize("which", ("count", "fragments"))
def test_reframe_skips(T, which, pattern):
    from kuma_amd import kmws
    src, offs, lens0, in_keys, flags0, out_keys = skip_batch(which)
    lens, flags = skip_pattern(pattern, lens0.astype(np.int64), flags0)
    n = len(lens)
    sk = (flags & SKIP) != 0
    offs = np.asarray(offs).astype(np.int64).copy()
    ref_offs, ref_lens = offs.copy(), lens.copy()
    if pattern == "wild_descriptors":  # skipped frames pointing far outside src: their payload is never read
        offs[sk] = (1 << 46) + 977 * np.arange(int(sk.sum()))
        lens[sk] = np.resize(np.array([0xFFFFFFFF, 1 << 31, 70000, 4096, 126, 1], dtype=np.int64), int(sk.sum()))
    want, want_off = reference(src, ref_offs, ref_lens, in_keys, flags, out_keys)
    assert np.all(np.diff(want_off)[sk] == 0) and np.all(np.diff(want_off)[~sk] >= 2)
    if pattern == "all":
        assert len(want) == 0
    if pattern == "run65_on_chunk_boundary":
        assert want_off[n // 3] % CHUNK == 0 and want_off[n // 3] > 0 and want_off[n // 3 + 70] == want_off[n // 3]
    if pattern == "run_straddles_boundary":
        mid = 2 * n // 3
        assert want_off[mid - 40] == want_off[mid] and want_off[mid + 1] == want_off[mid + 41]
        assert want_off[mid] // CHUNK != want_off[mid + 1] // CHUNK
    d_src = to_dev(T, src)
    descs = kmws.make_descs(offs, lens, in_keys.astype(np.int64))
    d_fl = T.from_numpy(flags.astype(np.uint16).view(np.int16)).cuda()
    d_ok = T.from_numpy(out_keys.view(np.int32)).cuda()
    for form in FORMS:
        cap = cap_for(form, n, len(want))
        buf, dst = guarded(T, cap)
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.reframe_batch(d_src, descs, d_fl, d_ok, dst, off, ws)
        check_output(T, (which, pattern, form), buf, dst, off, ws, want, want_off)


# ------------------------------ capacity ------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_reframe_capacity(T, form):
    from kuma_amd import kmws
    if form == "chunks":
        src, offs, lens, in_keys, flags, out_keys = mask_source("cap", pec.phase_batch(3, True, mixed_masks=True))
    else:  # a mean region above 16 KiB, so that total - 1 still selects the unit form
        lens = np.array([70000, 65536, 0, 33000, 126, 90001], dtype=np.int64)
        flags = np.full(len(lens), pec.FIN_BINARY | MASK, dtype=np.uint32)
        s, o, k = pec.layout_source("cap-units", lens)
        src, offs, lens, in_keys, flags, out_keys = mask_source("cap-units", (s, o, lens, flags, k))
    n = len(lens)
    flags = flags.copy()
    flags[1] |= SKIP
    want, want_off = reference(src, offs, lens, in_keys, flags, out_keys)
    total = len(want)
    d_src = to_dev(T, src)
    descs = kmws.make_descs(offs.astype(np.int64), lens, in_keys.astype(np.int64))
    d_fl = T.from_numpy(flags.astype(np.uint16).view(np.int16)).cuda()
    d_ok = T.from_numpy(out_keys.view(np.int32)).cuda()
    for cap, status in ((total - 1, 1), (total, 0)):
        assert (cap // n < pec.kChunkFormBelow) == (form == "chunks")
        buf, dst = guarded(T, cap)
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.reframe_batch(d_src, descs, d_fl, d_ok, dst, off, ws)
        T.cuda.synchronize()
        assert ws.status() == status, (form, cap)
        if status:
            assert bool((buf == FILL).all()), "stores with the output above dst_cap"
            with pytest.raises(kmws.KmwsError):
                kmws.reframe_batch(d_src, descs, d_fl, d_ok, dst, off, ws, check=True)
        else:
            check_output(T, (form, "cap == total"), buf, dst, off, ws, want, want_off)


# ------------------------------ the fused entry ------------------------------
def form_of(L):
    return hc.p7(L) if L <= 125 else hc.x16(L) if L <= 65535 else hc.x64(L)


@functools.lru_cache(maxsize=None)
def relay_wire(mode, errors):
    """About 300 frames as `mode` accepts them (masked for a server): TEXT, BINARY and CONTINUE, RSV1 on some, FIN or
    not, PING and PONG between them, gaps of 0-17 bytes before some headers; with `errors`, one record of every
    header-error kind of tests/header_cases.py between them and a truncated frame at the wire's end.
    Returns (wire, hdr_off, hc.Expected, number of error frames)."""
    rng = np.random.default_rng(0x52454C41 + 2 * mode + int(errors))
    mask = 1 if mode == hc.SERVER else 0
    key = lambda m: hc.random_key(rng) if m else b""  # noqa: E731
    lens = [0, 1, 5, 17, 125, 126, 127, 300, 1000, 4096, 4097, 65535, 65536, 70000]
    recs = []
    for i in range(300):
        if i % 7 == 3:
            b0, L = 0x80 | int(rng.choice([9, 10])), int(rng.choice([0, 3, 125]))
        else:
            L = int(rng.choice(lens[:11])) if i % 29 else int(rng.choice(lens[11:]))
            b0 = int(rng.integers(0, 2)) << 7 | (0x40 if i % 5 == 0 else 0) | int(rng.choice([0, 1, 2]))
        recs.append((hc.header_bytes(b0, mask, form_of(L), key(mask)), L))
    if errors:
        bad = [
            (hc.header_bytes(0x09, mask, hc.p7(3), key(mask)), 3),                    # control without FIN: 7
            (hc.header_bytes(0x89, mask, hc.x16(126), key(mask)), 126),               # control above 125: 7
            (hc.header_bytes(0x82, mask, hc.x16(125), key(mask)), 125),               # 126 class below 126: 6
            (hc.header_bytes(0x82, mask, hc.x64("8000000000000003"), key(mask)), 3),  # 127 class, bit 63: 6
            (hc.header_bytes(0x81, 1 - mask, hc.p7(9), key(1 - mask)), 9),            # the mask bit the mode rejects: 7
            (hc.header_bytes(0x82, mask, hc.x16(300), key(mask)), 40),                # overruns the next header: 5
        ]
        for k, rec in enumerate(bad):
            recs.insert(20 + 41 * k, rec)
        recs.append((hc.header_bytes(0x82, mask, hc.x16(500), key(mask)), 100))       # cut by the wire's end: 1
    parts, offs, cur = [], [], 0
    for i, (hdr, room) in enumerate(recs):
        gap = int(rng.integers(0, 18)) if i % 3 == 0 else 0
        parts += [rng.integers(0, 256, size=gap, dtype=np.uint8), np.frombuffer(hdr, np.uint8),
                  rng.integers(0, 256, size=room, dtype=np.uint8)]
        offs.append(cur + gap)
        cur += gap + len(hdr) + room
    wire = np.concatenate(parts)
    hdr_off = np.array(offs, dtype=np.int64)
    e = hc.Expected(wire, len(wire), hdr_off, mode)
    nbad = int((e.err != 0).sum())
    assert nbad == (7 if errors else 0), (mode, errors, e.err[e.err != 0])
    if errors:
        assert sorted(set(e.err[e.err != 0].tolist())) == [1, 5, 6, 7]
    return wire, hdr_off, e, nbad


@pytest.mark.parametrize("relay", (0x0007, 0xFFFF, 0x0002))
@pytest.mark.parametrize("errors", (False, True), ids=("clean", "errors"))
@pytest.mark.parametrize("mode", (hc.SERVER, hc.CLIENT), ids=("server", "client"))
def test_unpack_reframe(T, mode, errors, relay):
    from kuma_amd import kmws
    wire, hdr_off, e, nbad = relay_wire(mode, errors)
    n = len(hdr_off)
    opcode = e.flags & 0x0F
    skip = (e.err != 0) | (((relay >> opcode) & 1) == 0)
    assert 0 < int(skip.sum()) < n or relay == 0xFFFF
    rng = np.random.default_rng(relay + mode)
    out_keys = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    d_wire = to_dev(T, wire)
    d_hdr = T.from_numpy(hdr_off).cuda()
    d_ok = T.from_numpy(out_keys.view(np.int32)).cuda()
    want_desc = T.from_numpy(e.desc()).cuda()
    for out_mask in (0, 1):
        oflags = ((e.flags & 0xFF) | (MASK if out_mask else 0) | np.where(skip, SKIP, 0)).astype(np.uint32)
        # the composition: kmws_reframe_batch's reference on out_desc and those flags, on the same wire
        want, want_off = reference(wire, e.off, e.len, e.key, oflags, out_keys)
        for keys in ((d_ok, out_keys), (None, None)) if out_mask else ((d_ok, out_keys),):
            if keys[1] is None:
                want, want_off = reference(wire, e.off, e.len, e.key, oflags, None)
            for form in FORMS:
                cap = cap_for(form, n, len(want))
                buf, dst = guarded(T, cap)
                off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
                ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
                fd = T.full((n, 2), -1, dtype=T.int64, device="cuda")
                ff = T.full((n,), -1, dtype=T.int16, device="cuda")
                fe = T.full((n,), 99, dtype=T.uint8, device="cuda")
                kmws.unpack_reframe(d_wire, d_hdr, mode, fd, ff, fe, relay, out_mask, keys[0], dst, off, ws,
                                    wire_len=len(wire))
                tag = (mode, errors, hex(relay), out_mask, form)
                check_output(T, tag, buf, dst, off, ws, want, want_off, status=2 if nbad else 0)
                assert T.equal(fd, want_desc), tag
                assert np.array_equal(ff.cpu().numpy().view(np.uint16).astype(np.int64), e.flags), tag
                assert np.array_equal(fe.cpu().numpy(), e.err), tag
                # ... and what kmws_reframe_batch itself writes from those outputs
                buf2, dst2 = guarded(T, cap)
                off2 = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
                ws2 = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
                kmws.reframe_batch(d_wire, fd, T.from_numpy(oflags.astype(np.uint16).view(np.int16)).cuda(), keys[0],
                                   dst2, off2, ws2)
                check_output(T, tag + ("two-step",), buf2, dst2, off2, ws2, want, want_off)
    if errors:
        with pytest.raises(kmws.KmwsError) as ei:
            kmws.unpack_reframe(d_wire, d_hdr, mode, fd, None, None, relay, 0, None, dst, off, ws, wire_len=len(wire),
                                check=True)
        assert ei.value.ws_status == 2


# ------------------------------ fuzz ------------------------------
FUZZ_LENS = [0] + list(range(1, 18)) + [125, 126, 127, 300, 4095, 4096, 4097, 65535, 65536, 70000]
FUZZ_BYTES = 8 << 20


@pytest.mark.parametrize("block", range(8))
def test_reframe_fuzz(T, block):
    """200 seeded batches (25 per block) of 1-400 frames; payloads anywhere in the source, overlapping or not;
    incoming and outgoing masks random; at most a quarter of a batch skipped."""
    for seed in range(25 * block, 25 * block + 25):
        rng = np.random.default_rng(0xF022 + seed)
        n = int(rng.integers(1, 401))
        lens = rng.choice(FUZZ_LENS, size=n).astype(np.int64)
        big = np.flatnonzero(lens >= 65535)
        budget = FUZZ_BYTES - int(lens[lens < 65535].sum()) - 14 * n
        for k, f in enumerate(big):  # the large ones capped so that the batch stays under 8 MiB
            if (k + 1) * 70000 > budget:
                lens[f] = int(rng.choice(FUZZ_LENS[:24]))
        src_len = int(max(1 << 12, min(int(lens.sum()), 1 << 20), int(lens.max()) + 64))
        src = rng.integers(0, 256, size=src_len, dtype=np.uint8)
        offs = np.array([rng.integers(0, src_len - int(L) + 1) for L in lens], dtype=np.int64)
        in_keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        in_keys[rng.integers(0, 4, size=n) == 0] = 0
        out_keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        flags = (rng.integers(0, 256, size=n) | (rng.integers(0, 2, size=n) << 8)).astype(np.uint32)
        nskip = int(rng.integers(0, n // 4 + 1))
        flags[rng.permutation(n)[:nskip]] |= SKIP
        want, want_off = reference(src, offs, lens, in_keys, flags, out_keys)
        assert len(want) > 0 and len(want) <= FUZZ_BYTES
        run_reframe(T, src, offs, lens, in_keys, flags, out_keys, tag=("fuzz", seed))


# ------------------------------ capture ------------------------------
def test_reframe_graph_replay(T):
    """One kmws_reframe_batch call captured on a single stream and replayed twice on refreshed source bytes."""
    from kuma_amd import kmws
    rng = np.random.default_rng(0x47524146)
    n = 600
    lens = rng.choice([0, 1, 3, 125, 126, 1000, 4096, 65535, 65536, 70001], size=n).astype(np.int64)
    offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16 + 16)[:-1]]).astype(np.int64)
    src_len = int(offs[-1] + lens[-1] + 64)
    in_keys = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    out_keys = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    flags = (rng.integers(0, 2, size=n) << 7 | rng.choice([0, 1, 2], size=n) | rng.integers(0, 2, size=n) << 8).astype(
        np.uint32)
    flags[::9] |= SKIP
    total = len(reference(np.zeros(src_len, np.uint8), offs, lens, in_keys, flags, out_keys)[0])
    d_src = T.zeros(src_len + 16, dtype=T.uint8, device="cuda")
    descs = kmws.make_descs(offs, lens, in_keys.astype(np.int64))
    d_fl = T.from_numpy(flags.astype(np.uint16).view(np.int16)).cuda()
    d_ok = T.from_numpy(out_keys.view(np.int32)).cuda()
    buf, dst = guarded(T, total + 16)
    off = T.zeros(n + 1, dtype=T.int64, device="cuda")
    ws = kmws.Workspace(kmws.reframe_workspace_size(n, total + 16))

    def call():
        kmws.reframe_batch(d_src, descs, d_fl, d_ok, dst, off, ws)

    s = T.cuda.Stream()
    s.wait_stream(T.cuda.current_stream())
    with T.cuda.stream(s):  # warm (and load every kernel) before capture
        call()
    T.cuda.current_stream().wait_stream(s)
    T.cuda.synchronize()
    g = T.cuda.CUDAGraph()
    with T.cuda.graph(g):
        call()
    T.cuda.synchronize()
    for rep in range(2):
        src = np.random.default_rng(rep).integers(0, 256, size=src_len, dtype=np.uint8)
        want, want_off = reference(src, offs, lens, in_keys, flags, out_keys)
        buf.fill_(FILL)
        off.fill_(-1)
        d_src[:src_len].copy_(T.from_numpy(src))
        g.replay()
        check_output(T, ("replay", rep), buf, dst, off, ws, want, want_off)
