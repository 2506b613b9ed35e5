"""Every device batch entry with source, wire and output offsets past 2^31 and
2^32 bytes, byte for byte against the oracle.

The batches are the periodic ones of tests/far_offset_cases.py (proved on the
CPU by tests/test_far_offset_cases.py): one period of frames whose images the
oracle computed, repeated until source and output pass 2^32 + 2^27 bytes, with
a front that puts a named thing on byte 2^32 (or 2^31).  Every run asserts a
clean workspace status, every output offset against the numpy cumsum, every
output byte against the broadcast period image (compared on the device in row
slices; a failure reports the first wrong byte's absolute offset and which of
2^31 / 2^32 it lies past), dst past the total still the fill, every in-place
byte outside the payloads unchanged, the per-frame outputs against the period's
values at i % P -- and, from the descriptor arrays, that the run's source and
output offsets do exceed 2^32.

The copy form (chunks / units) follows from dst_cap alone, asserted with
pec.use_chunks: the "chunk" period has a mean region under 16 KiB, the "unit"
period at or above it.

Offset mutants: one 64-bit offset per kernel family masked to its low 32 bits
(`& 0xFFFFFFFFull`; never sign-extended, never leaving the allocation: a wrong
address inside the same buffer), each built from a scratch copy of the sources
and run once on an MI355X against the payload_first_byte-x32 cases of this
file.  The tests that failed:

  the unmask tile base (tile_rsrc's base + lo, kmws_unmask.hip only)
      -> test_in_place_entry[unmask_batch-default / -grouped_runs / -split],
         [unpack_unmask]
  the UTF-8 tile base, fused pass (the same line, kmws_utf8.hip only)
      -> test_in_place_entry[unmask_utf8_batch], [unpack_unmask_utf8]
  the UTF-8 tile base, read-only pass (utf8_payload_kernel's own base + lo)
      -> test_in_place_entry[utf8_validate-masked], [utf8_validate-plain]
  geom_at's source offset (sdel = x.off - p0)
      -> test_copy_entry[*-units], all 11 entries
  the unit copy's output address (copy wave's dst + a)
      -> test_copy_entry[*-units], all 11 entries
  the chunk copy's A0
      -> test_copy_entry[*-chunks] of encode_batch, gather_unmask,
         unpack_gather, reframe_batch and unpack_reframe (masked and unmasked);
         the four validating forms passed: a chunk whose words all turn into
         boundary words is handed to chunk_dense_kernel there, which computes
         its own offsets, so the mutant only slows them down
  the chunk copy's A0 and chunk_dense_kernel's store address together
      -> test_copy_entry[*-chunks], all 11 entries
  unpack_one's wire offset (h = hdr_off[f])
      -> test_in_place_entry[unpack_headers], [unpack_unmask],
         [unpack_unmask_utf8]; test_copy_entry of unpack_gather,
         unpack_reframe (both), unpack_gather_utf8, unpack_reframe_utf8 in
         both forms
  walk_step's position (the load address wire + p)
      -> test_in_place_entry[find_headers_streams]

The seven families of the issue at once against the suite as it was before this file: 1196 passed,
3 failed -- test_encode_4k_frames_past_4_gib[0] and [20000] (the chunk form's
A0) and test_resident_large_jobs_write_through_while_a_device_batch_runs (an
8 GiB kmws_unmask_batch under the device checker).  Nothing failed for the
other five families.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import far_offset_cases as foc  # noqa: E402
import pack_edge_cases as pec  # noqa: E402

pytestmark = pytest.mark.gpu
FILL, GUARD, SLACK = 0xEE, 64, 4096
X31, X32 = foc.X31, foc.X32
FORMS = {"chunks": "chunk", "units": "unit"}  # form -> the period whose mean region selects it

# (lead, boundary) of the in-place and wire-walking entries, and of the copy entries
IN_PLACE_LEADS = [(lead, X32) for lead in foc.LEADS] + [("payload_first_byte", X31)]
COPY_LEADS = [("payload_first_byte", X32), ("header_straddles", X32), ("key_phase_1", X32)]
COPY_UTF8_LEADS = COPY_LEADS + [("utf8_char_straddles", X32), ("utf8_bad_at", X32)]


def lead_id(v):
    return f"{v[0]}-x{v[1].bit_length() - 1}" if isinstance(v, tuple) else None


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    yield torch
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def free_after_each(T):
    yield
    T.cuda.empty_cache()


@functools.lru_cache(maxsize=16)
def layout(name, space, lead, X):
    return foc.Layout(foc.period(name), space, lead, X)


# ------------------------------ device helpers ------------------------------
def dev(T, a):
    return T.from_numpy(np.ascontiguousarray(a)).cuda()


def i16(T, a):
    return dev(T, np.asarray(a).astype(np.uint16).view(np.int16))


def i32(T, a):
    return dev(T, np.asarray(a).astype(np.uint32).view(np.int32))


def descs_of(T, off, lens, keys):
    from kuma_amd import kmws
    return kmws.make_descs(np.asarray(off, dtype=np.int64), np.asarray(lens, dtype=np.int64),
                           np.asarray(keys).astype(np.int64))


def fill_tiled(T, buf, front, img, reps, bad_row, bad_img):
    """buf[:] = front | img x reps (row bad_row: bad_img) | GAP_FILL to the end."""
    S = len(img)
    a = len(front)
    if a:
        buf[:a] = dev(T, front)
    rows = buf[a:a + reps * S].view(reps, S)
    rows.copy_(dev(T, img).expand(reps, S))
    if bad_row is not None:
        rows[bad_row] = dev(T, bad_img)
    buf[a + reps * S:] = foc.GAP_FILL


def first_wrong(T, ne, base):
    p = base + int(ne.reshape(-1).nonzero()[0])
    return f"first wrong byte at {p} (past 2^31: {p >= X31}, past 2^32: {p >= X32})"


def assert_tiled(T, what, buf, front, img, reps, bad_row, bad_img):
    """buf == front | img x reps, compared on the device in row slices."""
    S = len(img)
    a = len(front)
    if a:
        ne = buf[:a] != dev(T, front)
        assert not bool(ne.any()), (what, "front", first_wrong(T, ne, 0))
    rows = buf[a:a + reps * S].view(reps, S)
    d_img = dev(T, img)
    d_bad = dev(T, bad_img) if bad_row is not None else None
    step = max(1, (192 << 20) // S)
    for r0 in range(0, reps, step):
        blk = rows[r0:r0 + step]
        ne = blk != d_img
        if bad_row is not None and r0 <= bad_row < r0 + step:
            ne[bad_row - r0] = blk[bad_row - r0] != d_bad
        assert not bool(ne.any()), (what, first_wrong(T, ne, a + r0 * S))
        del ne


def source(T, L, masked=True):
    """The source arena on the device: src_bytes of batch, then 64 gap bytes."""
    buf = T.empty(L.src_bytes + 64 + (-L.src_bytes) % 16, dtype=T.uint8, device="cuda")
    fm, fp, _ = L.front_images()
    bad = L.period_images(True) if L.bad_row is not None else (None, None, None)
    k = 0 if masked else 1
    fill_tiled(T, buf, (fm, fp)[k], L.period_images()[k], L.reps, L.bad_row, bad[k])
    return buf


def assert_source(T, what, L, buf, masked):
    fm, fp, _ = L.front_images()
    bad = L.period_images(True) if L.bad_row is not None else (None, None, None)
    k = 0 if masked else 1
    assert_tiled(T, what, buf, (fm, fp)[k], L.period_images()[k], L.reps, L.bad_row, bad[k])
    assert bool((buf[L.src_bytes:] == foc.GAP_FILL).all()), (what, "bytes past the source")


def assert_past_4_gib(L):
    """The run's own arrays: payload and header offsets (and output offsets) past 2^32."""
    assert L.pay_off[-1] > X32 and L.hdr_off[-1] > X32 and L.src_bytes > X32 + (1 << 27) - 1
    assert int(np.sum(L.pay_off < X31)) and int(np.sum((L.pay_off >= X31) & (L.pay_off < X32)))
    if L.copy:
        assert L.out_off[-2] > X32 and L.out_bytes >= foc.MIN_SPAN


def want_records(T, L):
    """out_desc / out_flags of the header parse: the period's values at i % P."""
    return descs_of(T, L.pay_off, L.lens, L.keys), i16(T, L.flags_in())


def header_outputs(T, n):
    return (T.full((n, 2), -1, dtype=T.int64, device="cuda"), T.full((n,), -1, dtype=T.int16, device="cuda"),
            T.full((n,), 99, dtype=T.uint8, device="cuda"))


def assert_records(T, what, L, od, of, oe):
    wd, wf = want_records(T, L)
    assert T.equal(od, wd), (what, "out_desc", int((od != wd).any(dim=1).nonzero()[0]))
    assert T.equal(of, wf), (what, "out_flags", int((of != wf).nonzero()[0]))
    assert int(oe.count_nonzero()) == 0, (what, "out_err", int(oe.nonzero()[0]))


def utf8_outputs(T, n):
    return T.full((n,), 0xEE, dtype=T.uint8, device="cuda"), T.full((1, 8), 0xEE, dtype=T.uint8, device="cuda")


def assert_verdicts(T, what, L, out, carry):
    want = dev(T, L.verdicts)
    assert T.equal(out, want), (what, "verdicts", int((out != want).nonzero()[0]))
    assert int(carry.count_nonzero()) == 0, (what, "carry_out", carry.cpu().tolist())


# ------------------------------ in-place and wire-walking entries ------------------------------
def run_unmask(T, L, schedule):
    from kuma_amd import kmws
    buf = source(T, L)
    d = descs_of(T, L.pay_off, L.lens, L.keys)
    ws = kmws.Workspace(kmws.unmask_workspace_size(L.src_bytes))
    kmws.unmask_plan(d, ws, L.src_bytes)
    kmws.unmask_apply(buf, d, ws, L.src_bytes, schedule=schedule)
    T.cuda.synchronize()
    assert ws.status() == 0
    assert_source(T, "unmask", L, buf, masked=False)


def run_unpack_headers(T, L, fused):
    from kuma_amd import kmws
    buf = source(T, L)
    od, of, oe = header_outputs(T, L.n)
    hdr = dev(T, L.hdr_off)
    if fused:
        ws = kmws.Workspace(kmws.unmask_workspace_size(L.src_bytes))
        kmws.unpack_unmask(buf, hdr, kmws.SERVER, od, of, oe, ws, wire_len=L.src_bytes)
    else:
        ws = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
        kmws.unpack_headers(buf, hdr, kmws.SERVER, od, of, oe, ws, wire_len=L.src_bytes)
    T.cuda.synchronize()
    assert ws.status() == 0
    assert_records(T, "unpack", L, od, of, oe)
    assert_source(T, "unpack", L, buf, masked=not fused)


def run_find_headers_streams(T, L):
    """One stream per period (its wire and the gap after it, which holds no
    whole frame): streams before 2^32, one across it, streams wholly past it.
    Reference: kmws_find_headers on the period plus the offset arithmetic."""
    from kuma_amd import kmws
    p = L.p
    buf = source(T, L)
    cap = p.P + 3
    want_h, want_used = kmws.find_headers(p.src_masked, cap)  # the gap's first bytes read as one more, cut, header
    k = len(want_h)
    assert want_h[:p.P] == p.hdr_off.tolist() and want_used == p.S_wire and p.P <= k < cap
    start = L.front_src + np.arange(L.reps + 1, dtype=np.int64) * p.S_src
    assert start[-1] == L.src_bytes
    assert np.any((start[:-1] < X32) & (start[1:] > X32)) and np.sum(start[:-1] > X32) > 100
    hdr = T.full((L.reps, cap), -7, dtype=T.int64, device="cuda")
    hdr, n_out, consumed = kmws.find_headers_streams(buf, dev(T, start), cap, wire_len=L.src_bytes, hdr=hdr)
    T.cuda.synchronize()
    assert bool((n_out == k).all()), int((n_out != k).nonzero()[0])
    assert bool((consumed == want_used).all()), int((consumed != want_used).nonzero()[0])
    want = dev(T, start[:-1, None] + np.array(want_h, dtype=np.int64)[None, :])
    assert T.equal(hdr[:, :k], want), int((hdr[:, :k] != want).any(dim=1).nonzero()[0])
    assert bool((hdr[:, k:] == -7).all())
    assert T.equal(hdr[:, :p.P].reshape(-1), dev(T, L.hdr_off))  # the list the unpack entries take
    assert_source(T, "find_headers_streams", L, buf, masked=True)


def run_pack_headers(T, L):
    """Header slots, lengths and the chained wire_off of the encode image's frames
    (masked and unmasked mixed) at the source's descriptors."""
    from kuma_amd import kmws
    p = L.p
    n, reps = L.n, L.reps
    enc, hl, fl = p.out["encode"]
    S, h, pay = p.geom("encode")
    slots = np.zeros((p.P, 16), dtype=np.uint8)
    for j in range(p.P):
        slots[j, :hl[j]] = enc[h[j]:pay[j]]
    keys = np.where(p.enc_mask, p.out_keys, 0)
    d = descs_of(T, L.pay_off, L.lens, np.tile(keys, reps))
    hdr = T.full((16 * n,), FILL, dtype=T.uint8, device="cuda")
    hlen = T.full((n,), FILL, dtype=T.uint8, device="cuda")
    woff = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    ws = kmws.Workspace(kmws.pack_headers_workspace_size(n))
    kmws.pack_headers(d, i16(T, np.tile(fl, reps)), hdr, hlen, woff, ws)
    T.cuda.synchronize()
    assert ws.status() == 0
    want_off = np.concatenate([[0], np.cumsum(np.tile(hl + p.lens, reps))]).astype(np.int64)
    assert want_off[-1] > X32 and want_off[-1] == reps * S
    assert T.equal(woff, dev(T, want_off)), int((woff != dev(T, want_off)).nonzero()[0])
    assert T.equal(hdr.view(reps, p.P * 16), dev(T, slots.reshape(-1)).expand(reps, p.P * 16))
    assert T.equal(hlen.view(reps, p.P), dev(T, hl.astype(np.uint8)).expand(reps, p.P))


def run_utf8_validate(T, L, masked):
    from kuma_amd import kmws
    buf = source(T, L, masked=masked)
    d = descs_of(T, L.pay_off, L.lens, L.keys)
    out, carry = utf8_outputs(T, L.n)
    ws = kmws.Workspace(kmws.utf8_workspace_size(L.src_bytes, L.n, 1))
    kmws.utf8_validate(buf, d, i16(T, L.flags_in()), out, ws, span=L.src_bytes, masked=masked, carry_out=carry)
    T.cuda.synchronize()
    assert ws.status() == 0
    assert_verdicts(T, "utf8_validate", L, out, carry)
    assert_source(T, "utf8_validate", L, buf, masked=masked)  # only read


def run_unmask_utf8(T, L, fused):
    from kuma_amd import kmws
    buf = source(T, L)
    out, carry = utf8_outputs(T, L.n)
    ws = kmws.Workspace(kmws.unmask_utf8_workspace_size(L.src_bytes, L.n, 1))
    if fused:
        od, of, oe = header_outputs(T, L.n)
        kmws.unpack_unmask_utf8(buf, dev(T, L.hdr_off), kmws.SERVER, od, of, oe, out, ws, wire_len=L.src_bytes,
                                carry_out=carry)
    else:
        d = descs_of(T, L.pay_off, L.lens, L.keys)
        kmws.unmask_utf8(buf, d, i16(T, L.flags_in()), out, ws, span=L.src_bytes, carry_out=carry)
    T.cuda.synchronize()
    assert ws.status() == 0
    if fused:
        assert_records(T, "unpack_unmask_utf8", L, od, of, oe)
    assert_verdicts(T, "unmask_utf8", L, out, carry)
    assert_source(T, "unmask_utf8", L, buf, masked=False)


def _sched(name):
    from kuma_amd import kmws
    return {"default": None, "grouped_runs": kmws.SCHED_GROUPED_RUNS, "split": kmws.SCHED_SPLIT4}[name]


IN_PLACE = {
    "unmask_batch-default": lambda T, L: run_unmask(T, L, _sched("default")),
    "unmask_batch-grouped_runs": lambda T, L: run_unmask(T, L, _sched("grouped_runs")),
    "unmask_batch-split": lambda T, L: run_unmask(T, L, _sched("split")),
    "unpack_headers": lambda T, L: run_unpack_headers(T, L, fused=False),
    "unpack_unmask": lambda T, L: run_unpack_headers(T, L, fused=True),
    "find_headers_streams": run_find_headers_streams,
    "pack_headers": run_pack_headers,
    "utf8_validate-masked": lambda T, L: run_utf8_validate(T, L, masked=True),
    "utf8_validate-plain": lambda T, L: run_utf8_validate(T, L, masked=False),
    "unmask_utf8_batch": lambda T, L: run_unmask_utf8(T, L, fused=False),
    "unpack_unmask_utf8": lambda T, L: run_unmask_utf8(T, L, fused=True),
}


@pytest.mark.parametrize("lead", IN_PLACE_LEADS, ids=lead_id)
@pytest.mark.parametrize("entry", list(IN_PLACE))
def test_in_place_entry(T, entry, lead):
    L = layout("chunk", "src", *lead)
    assert_past_4_gib(L)
    IN_PLACE[entry](T, L)


# ------------------------------ copy entries ------------------------------
def run_copy(T, L, entry, form):
    """One copy entry on layout L: returns nothing, asserts everything."""
    from kuma_amd import kmws
    n = L.n
    cap = L.out_bytes + SLACK
    assert pec.use_chunks(n, cap) == (form == "chunks"), (form, n, cap)
    utf8 = "utf8" in entry
    unpack = entry.startswith("unpack")
    buf = source(T, L, masked=L.space != "encode")  # encode reads plain payloads, the others the masked wire
    guard = T.full((GUARD + cap + GUARD,), FILL, dtype=T.uint8, device="cuda")
    dst = guard[GUARD:GUARD + cap]
    off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    out, carry = utf8_outputs(T, n) if utf8 else (None, None)
    od, of, oe = header_outputs(T, n) if unpack else (None, None, None)
    hdr = dev(T, L.hdr_off) if unpack else None
    d = None if unpack else descs_of(T, L.pay_off, L.lens, L.keys)
    fl_out = L.flags_out() if L.space != "gather" else None
    ok = np.where(fl_out & foc.MASK, L.out_keys, 0) if fl_out is not None else None
    W = L.src_bytes
    if entry == "encode_batch":
        d = descs_of(T, L.pay_off, L.lens, ok)
        ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
        kmws.encode_batch(buf, d, i16(T, fl_out), dst, off, ws)
    elif entry == "gather_unmask":
        ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
        kmws.gather_unmask(buf, d, dst, off, ws)
    elif entry == "unpack_gather":
        ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
        kmws.unpack_gather(buf, hdr, kmws.SERVER, od, of, oe, dst, off, ws, wire_len=W)
    elif entry == "reframe_batch":
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.reframe_batch(buf, d, i16(T, fl_out), i32(T, L.out_keys), dst, off, ws)
    elif entry == "unpack_reframe":
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.unpack_reframe(buf, hdr, kmws.SERVER, od, of, oe, 0xFFFF, L.space == "reframe_m", i32(T, L.out_keys), dst,
                            off, ws, wire_len=W)
    elif entry == "gather_unmask_utf8":
        ws = kmws.Workspace(kmws.gather_utf8_workspace_size(n, cap, 1))
        kmws.gather_unmask_utf8(buf, d, i16(T, L.flags_in()), dst, off, out, ws, carry_out=carry)
    elif entry == "unpack_gather_utf8":
        ws = kmws.Workspace(kmws.gather_utf8_workspace_size(n, cap, 1))
        kmws.unpack_gather_utf8(buf, hdr, kmws.SERVER, od, of, oe, dst, off, out, ws, wire_len=W, carry_out=carry)
    elif entry == "reframe_utf8_batch":
        ws = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap, 1))
        kmws.reframe_utf8(buf, d, i16(T, fl_out), i32(T, L.out_keys), dst, off, out, ws, carry_out=carry)
    elif entry == "unpack_reframe_utf8":
        ws = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap, 1))
        kmws.unpack_reframe_utf8(buf, hdr, kmws.SERVER, od, of, oe, 0xFFFF, L.space == "reframe_m",
                                 i32(T, L.out_keys), dst, off, out, ws, wire_len=W, carry_out=carry)
    else:
        raise ValueError(entry)
    T.cuda.synchronize()
    what = (entry, form, L.space, L.lead)
    assert ws.status() == 0, what
    want_off = dev(T, L.out_off)
    assert T.equal(off, want_off), what + ("first wrong offset", int((off != want_off).nonzero()[0]))
    _, _, fo = L.front_images()
    bad_img = L.period_images(True)[2] if L.bad_row is not None else None
    assert_tiled(T, what, dst[:L.out_bytes], fo, L.period_images()[2], L.reps, L.bad_row, bad_img)
    assert bool((dst[L.out_bytes:] == FILL).all()), what + ("dst past the total",)
    assert bool((guard[:GUARD] == FILL).all()) and bool((guard[GUARD + cap:] == FILL).all()), what + ("guards",)
    if unpack:
        assert_records(T, what, L, od, of, oe)
    if utf8:
        assert_verdicts(T, what, L, out, carry)
    assert_source(T, what, L, buf, masked=L.space != "encode")  # the source is only read


COPY = [  # (entry, output space)
    ("encode_batch", "encode"),
    ("gather_unmask", "gather"), ("unpack_gather", "gather"),
    ("reframe_batch", "reframe_m"), ("reframe_batch", "reframe_u"),
    ("unpack_reframe", "reframe_m"), ("unpack_reframe", "reframe_u"),
]
COPY_UTF8 = [
    ("gather_unmask_utf8", "gather"), ("unpack_gather_utf8", "gather"),
    ("reframe_utf8_batch", "reframe_m"), ("unpack_reframe_utf8", "reframe_u"),
]
COPY_CASES = [(e, s, lead) for e, s in COPY for lead in COPY_LEADS] + \
             [(e, s, lead) for e, s in COPY_UTF8 for lead in COPY_UTF8_LEADS]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("entry,space,lead", COPY_CASES,
                         ids=[f"{e}-{s}-{lead_id(lead)}" for e, s, lead in COPY_CASES])
def test_copy_entry(T, entry, space, lead, form):
    L = layout(FORMS[form], space, *lead)
    assert_past_4_gib(L)
    run_copy(T, L, entry, form)
