"""Header-rule parity of the device frame parse and of both header-chain walks
against the oracle decoder (kuma's WSHandler::decodeFrame restated): the
corpora, records and streams of tests/header_cases.py (whose claims
tests/test_header_cases.py proves on the CPU) through kmws_unpack_headers,
kmws_unpack_unmask, kmws_unpack_gather and kmws_find_headers_streams.  Every
expectation comes from header_cases.expect / walk_expect, i.e. from the oracle,
never from the library; outputs are pre-filled with a sentinel.

Which case pins which rule and which read path of `unpack_one`
(kmws_frame_parse.hpp) and `walk_step` / `walk_headers_kernel` (kmws_pack.hip):

  test_unpack_headers_corpus   every header rule on the FUNNEL path (one pair of
                               aligned 16-byte loads shifted by h & 15): all 256
                               values of byte 0 x MASK x five length forms, and
                               eight flag bytes x MASK x every length form
                               (126-class below 126, the 127-class quirk and
                               rejection patterns, the 10 MiB cap and cap + 1),
                               each at all 16 phases, in both modes: non-FIN
                               control, control with plen > 125, the three
                               127-class rejections, CLIENT-rejects-masked,
                               SERVER-rejects-unmasked, overrun (err 5), and
                               truncation (err 1) at the wire's end.  out_flags
                               for good AND error frames; status 2 / 0.
  test_fused_forms_corpus      the same verdicts from the plan kernel of
                               kmws_unpack_unmask and the scan of
                               kmws_unpack_gather; the wire byte for byte after
                               the in-place decode (error frames still masked,
                               gaps and headers untouched); dst_off, dst[:total]
                               and the fill behind it for the gather.
  test_header_tail_sweep       the BYTE path (header within 32 bytes of the
                               wire's end) and the truncation order: a wire cut
                               at every byte of each header length 2..14 and of
                               each error record, at every phase, 0xFF behind
                               wire_len.  Pins HDR1 (a non-FIN control byte alone
                               is err 7, not 1), h + 2 + ext, h + hl, the key
                               bytes at hl - 4, and err 1 against err 6 / 7 order.
  test_unpack_headers_unaligned_wire  the absolute-address window (a16, end16)
                               with the wire pointer at 1, 7 and 15 mod 16.
  test_walk_streams_edges      walk_step's stop rules (truncation at every byte
                               of a 14-byte header, CLOSE, 126-class 0 and 125,
                               127-class bit 63 and cap + 1, one byte, empty) on
                               both read paths; the 16-offset buffer and its
                               flush `out[n - cnt + j]` at 15..33 frames and caps
                               1..100 (rows untouched past n_out); the 256-lane
                               block edge at 255 / 256 / 257 streams; device walk
                               == host walk == oracle.

One-condition mutants of a scratch copy of the source (never committed; all
only misread bytes inside the tests' tensors), each built once, and the tests
that caught them on an MI355X when this file was written:

  unpack_one `len < 126` -> `len < 125`      the corpus tests (both modes, all three
                                             entries), the unaligned wire, the tail sweep
                                             (x16_125: err 6 expected).
  unpack_one without `!fin && op >= 8`       the same six; tail sweep at control_not_fin.
  unpack_one `k0 = hl - 4` -> `hl - 3`       the SERVER corpus tests (every masked good
                                             frame's key), unaligned wire, tail sweep (hl6).
  ext_len127 without `& 31u`                 all seven tests (the walk shares ext_len127):
                                             the single-byte and quirk127 patterns.
  flush `j < cnt` -> `j + 1 < cnt`           test_walk_streams_edges (cap 1 first).  The
                                             `<=` form and an index one lower store outside
                                             the row or the buffer and were not built.
  unpack_one without the one-byte HDR1 rule  test_header_tail_sweep (control_not_fin cut 1):
                                             the parse as it was before these tests.
  walk_step without the `L < 126` stop       test_walk_streams_edges (x16_0, x16_125): the
                                             walk as it was before these tests.
  walk_step `a16 + 32 <= end16` -> `+ 16`    NOT caught, and cannot be by comparing outputs:
                                             the condition then always holds, the walk reads
                                             the 16 bytes behind the wire's last word, but
                                             every byte it uses is checked against the
                                             stream's end first (p + 2, p + 2 + ext), as on
                                             the funnel path of a stream that ends inside the
                                             wire.  Only the read itself differs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import header_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xEE
MODES = [pytest.param(hc.SERVER, id="server"), pytest.param(hc.CLIENT, id="client")]


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


def dev_wire(T, wire, shift=0, slack=64):
    """A device tensor holding `wire` at byte `shift`, 0xFF everywhere else
    (at least `slack` bytes behind it); returns (tensor, view from shift)."""
    size = (shift + len(wire) + slack + 31) // 16 * 16
    base = T.full((size,), 0xFF, dtype=T.uint8, device="cuda")
    base[shift:shift + len(wire)] = T.from_numpy(np.ascontiguousarray(wire)).cuda()
    return base, base[shift:]


def outputs(T, n):
    return (T.full((n, 2), -1, dtype=T.int64, device="cuda"), T.full((n,), -1, dtype=T.int16, device="cuda"),
            T.full((n,), 99, dtype=T.uint8, device="cuda"))


def assert_frames(what, got_desc, got_flags, got_err, want_desc, want_flags, want_err, label=None):
    """desc, flags and err of every frame; names the first frame that differs."""
    got = np.concatenate([np.asarray(got_desc, np.int64).reshape(-1, 2),
                          np.asarray(got_flags).astype(np.int64).reshape(-1, 1) & 0xFFFF,
                          np.asarray(got_err).astype(np.int64).reshape(-1, 1)], axis=1)
    want = np.concatenate([np.asarray(want_desc, np.int64).reshape(-1, 2),
                           np.asarray(want_flags, np.int64).reshape(-1, 1),
                           np.asarray(want_err).astype(np.int64).reshape(-1, 1)], axis=1)
    assert got.shape == want.shape, what
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        f = int(bad[0])
        cols = ("off", "len|key<<32", "flags", "err")
        diff = {c: (hex(int(g) & (2**64 - 1)), hex(int(w) & (2**64 - 1)))
                for c, g, w in zip(cols, got[f], want[f]) if g != w}
        pytest.fail(f"{what}: {len(bad)} of {len(got)} frames differ; first {f}"
                    f"{' ' + str(label(f)) if label else ''}: (got, want) {diff}")


def corpus_label(c):
    def label(f):
        k = c.kinds[c.kind_id[f]] if c.kind_id[f] >= 0 else "tail"
        return f"{k} at {int(c.hdr_off[f])} (phase {int(c.hdr_off[f]) % 16})"
    return label


def to_np(t):
    return t.cpu().numpy()


# ------------------------------ the corpora ------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_unpack_headers_corpus(T, mode):
    from kuma_amd import kmws
    c, e = hc.corpus(mode), hc.corpus_expected(mode)
    base, d_wire = dev_wire(T, c.wire)
    d_hdr = T.from_numpy(c.hdr_off).cuda()
    desc, flags, err = outputs(T, c.n)
    ws = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
    kmws.unpack_headers(d_wire, d_hdr, mode, desc, flags, err, ws, wire_len=c.wire_len)
    T.cuda.synchronize()
    assert_frames("kmws_unpack_headers", to_np(desc), to_np(flags), to_np(err), e.desc(), e.flags, e.err,
                  corpus_label(c))
    assert e.err.any() and ws.status() == 2
    # only the good frames (each still ends by the next header given, so the
    # oracle's verdicts stand): nothing may raise the status
    good = np.nonzero(e.err == 0)[0]
    desc, flags, err = outputs(T, len(good))
    kmws.unpack_headers(d_wire, T.from_numpy(c.hdr_off[good]).cuda(), mode, desc, flags, err, ws,
                        wire_len=c.wire_len)
    T.cuda.synchronize()
    assert_frames("good frames only", to_np(desc), to_np(flags), to_np(err), e.desc()[good], e.flags[good],
                  e.err[good], lambda f: corpus_label(c)(good[f]))
    assert ws.status() == 0


@pytest.mark.parametrize("mode", MODES)
def test_fused_forms_corpus(T, mode):
    from kuma_amd import kmws
    c, e = hc.corpus(mode), hc.corpus_expected(mode)
    W = c.wire_len
    base, d_wire = dev_wire(T, c.wire)
    d_hdr = T.from_numpy(c.hdr_off).cuda()
    good = np.nonzero((e.err == 0) & (e.len > 0))[0]
    # in place: good payloads become the oracle's, every other byte stays
    want = to_np(base).copy()
    for f in good:
        want[e.off[f]:e.off[f] + e.len[f]] = np.frombuffer(e.payload[f], np.uint8)
    w = base.clone()
    desc, flags, err = outputs(T, c.n)
    wsm = kmws.Workspace(kmws.unmask_workspace_size(W))
    kmws.unpack_unmask(w, d_hdr, mode, desc, flags, err, wsm, wire_len=W)
    T.cuda.synchronize()
    assert_frames("kmws_unpack_unmask", to_np(desc), to_np(flags), to_np(err), e.desc(), e.flags, e.err,
                  corpus_label(c))
    assert wsm.status() == 2
    got = to_np(w)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        f = int(np.searchsorted(c.hdr_off, at, side="right")) - 1
        pytest.fail(f"in-place decode: byte {at} differs, in the region of frame {f} {corpus_label(c)(max(f, 0))} "
                    f"(err {int(e.err[max(f, 0)])})")
    # gather: the oracle's payloads back to back
    total = int(e.len.sum())
    dst = T.full(((total + 64 + 15) // 16 * 16,), FILL, dtype=T.uint8, device="cuda")
    doff = T.full((c.n + 1,), -1, dtype=T.int64, device="cuda")
    desc, flags, err = outputs(T, c.n)
    wsg = kmws.Workspace(kmws.copy_workspace_size(c.n, dst.numel()))
    kmws.unpack_gather(d_wire, d_hdr, mode, desc, flags, err, dst, doff, wsg, wire_len=W)
    T.cuda.synchronize()
    assert_frames("kmws_unpack_gather", to_np(desc), to_np(flags), to_np(err), e.desc(), e.flags, e.err,
                  corpus_label(c))
    assert wsg.status() == 2
    assert np.array_equal(to_np(doff), np.concatenate([[0], np.cumsum(e.len)]))
    got = to_np(dst)
    assert got[:total].tobytes() == b"".join(e.payload[f] for f in good)
    assert np.all(got[total:] == FILL)
    assert T.equal(d_wire, base)  # the gather only reads the wire


def test_unpack_headers_unaligned_wire(T):
    """kmws_unpack_headers promises any alignment of the wire pointer: the
    SERVER corpus (a superset of its length sweep) at tensor offsets 1, 7, 15."""
    from kuma_amd import kmws
    c, e = hc.corpus(hc.SERVER), hc.corpus_expected(hc.SERVER)
    d_hdr = T.from_numpy(c.hdr_off).cuda()
    ws = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
    for shift in (1, 7, 15):
        base, d_wire = dev_wire(T, c.wire, shift=shift)
        assert d_wire.data_ptr() % 16 == shift
        desc, flags, err = outputs(T, c.n)
        kmws.unpack_headers(d_wire, d_hdr, hc.SERVER, desc, flags, err, ws, wire_len=c.wire_len)
        T.cuda.synchronize()
        assert_frames(f"wire at +{shift}", to_np(desc), to_np(flags), to_np(err), e.desc(), e.flags, e.err,
                      corpus_label(c))
        assert ws.status() == 2


# ------------------------------ the tail sweep ------------------------------
STRIDE = 192      # a row: phase (15) + the longest record (8 + 126) and 0xFF behind it
SLOT = 256        # per-launch slot of every output buffer


def _tail_rows(reduced):
    """Rows (wire images), per-row (wire_len, hdr offsets, mode, name) and the
    expectations of every frame of every row."""
    rows, meta, want = [], [], []
    for name, mode, frame, hl, _ in hc.tail_records():
        cuts = range(len(frame) + 1)
        if reduced:
            cuts = sorted({0, 1, 2, hl - 1, hl, len(frame) - 1, len(frame)})
        for phase in ((0, 1, 15) if reduced else range(16)):
            for cut in cuts:
                row, wl, offs = hc.tail_wire(frame, phase, cut, STRIDE)
                rows.append(row)
                meta.append((wl, offs, mode, f"{name} phase {phase} cut {cut}"))
                want.append([hc.expect_full(row, wl, offs, f, mode) for f in range(len(offs))])
    return np.stack(rows), meta, want


def _slots(T, count, nbytes, fill):
    return T.full((count * nbytes + 64,), fill, dtype=T.uint8, device="cuda")


def _tail_check(what, meta, want, desc, flags, err, status):
    desc = to_np(desc).view(np.int64).reshape(len(meta), -1)
    flags = to_np(flags).view(np.uint16).reshape(len(meta), -1)
    err = to_np(err).reshape(len(meta), -1)
    status = to_np(status).view(np.uint32).reshape(len(meta), -1)[:, 0]
    for i, ((wl, offs, mode, name), w) in enumerate(zip(meta, want)):
        n = len(offs)
        w_desc = [[x[1], x[2] | (x[3] << 32)] for x in w]
        assert_frames(f"{what}: {name}", desc[i, :2 * n].reshape(n, 2), flags[i, :n], err[i, :n],
                      np.array(w_desc, np.uint64).view(np.int64), [x[4] for x in w], [x[0] for x in w])
        assert status[i] == (2 if any(x[0] for x in w) else 0), (what, name, status[i])
        # nothing behind the n frames was written
        assert np.all(desc[i, 2 * n:] == -1) and np.all(flags[i, n:] == 0xFFFF) and np.all(err[i, n:] == 0xFF), name


def test_header_tail_sweep(T):
    from kuma_amd import kmws
    L = kmws.lib()
    # ---- kmws_unpack_headers: every cut at every phase ----
    rows, meta, want = _tail_rows(reduced=False)
    N = len(meta)
    assert N > 2000
    d_rows = T.from_numpy(np.concatenate([rows.reshape(-1), np.full(64, 0xFF, np.uint8)])).cuda()
    hdr = np.zeros((N, 2), np.int64)
    for i, (wl, offs, mode, name) in enumerate(meta):
        hdr[i, :len(offs)] = offs
    d_hdr = T.from_numpy(hdr).cuda()
    desc, flags, err, ws = (_slots(T, N, 64, 0xFF) for _ in range(4))
    for i, (wl, offs, mode, name) in enumerate(meta):
        st = L.kmws_unpack_headers(d_rows.data_ptr() + i * STRIDE, wl, d_hdr.data_ptr() + 16 * i, len(offs), mode,
                                   desc.data_ptr() + 64 * i, flags.data_ptr() + 64 * i, err.data_ptr() + 64 * i,
                                   ws.data_ptr() + 64 * i, 64, None)
        assert st == 0, name
    T.cuda.synchronize()
    _tail_check("kmws_unpack_headers", meta, want, desc[:N * 64], flags[:N * 64], err[:N * 64], ws[:N * 64])
    assert np.array_equal(to_np(d_rows)[:rows.size].reshape(rows.shape), rows)

    # ---- the reduced set through both fused forms ----
    rows, meta, want = _tail_rows(reduced=True)
    N = len(meta)
    flat = np.concatenate([rows.reshape(-1), np.full(64, 0xFF, np.uint8)])
    d_rows = T.from_numpy(flat).cuda()
    hdr = np.zeros((N, 2), np.int64)
    for i, (wl, offs, mode, name) in enumerate(meta):
        hdr[i, :len(offs)] = offs
    d_hdr = T.from_numpy(hdr).cuda()
    # in place
    w_rows = d_rows.clone()
    desc, flags, err = (_slots(T, N, 64, 0xFF) for _ in range(3))
    wsz = max(int(kmws.unmask_workspace_size(STRIDE)), 16)
    wsz = (wsz + 63) // 64 * 64
    ws = _slots(T, N, wsz, 0xFF)
    for i, (wl, offs, mode, name) in enumerate(meta):
        st = L.kmws_unpack_unmask(w_rows.data_ptr() + i * STRIDE, wl, d_hdr.data_ptr() + 16 * i, len(offs), mode,
                                  desc.data_ptr() + 64 * i, flags.data_ptr() + 64 * i, err.data_ptr() + 64 * i,
                                  ws.data_ptr() + wsz * i, wsz, -1, None)
        assert st == 0, name
    T.cuda.synchronize()
    status = ws[:N * wsz].reshape(N, wsz)[:, :4].contiguous()
    _tail_check("kmws_unpack_unmask", meta, want, desc[:N * 64], flags[:N * 64], err[:N * 64], status)
    want_rows = rows.copy()
    for i, w in enumerate(want):
        for x in w:
            if x[0] == 0 and x[2]:
                want_rows[i, x[1]:x[1] + x[2]] = np.frombuffer(x[5], np.uint8)
    got_rows = to_np(w_rows)[:rows.size].reshape(rows.shape)
    for i in range(N):
        assert np.array_equal(got_rows[i], want_rows[i]), f"in-place decode: {meta[i][3]}"
    assert np.all(to_np(w_rows)[rows.size:] == 0xFF)
    # gather
    desc, flags, err = (_slots(T, N, 64, 0xFF) for _ in range(3))
    gsz = (int(kmws.copy_workspace_size(2, SLOT)) + 255) // 256 * 256
    ws = _slots(T, N, gsz, 0xFF)
    dst = _slots(T, N, SLOT, FILL)
    doff = _slots(T, N, 64, 0xFF)
    for i, (wl, offs, mode, name) in enumerate(meta):
        st = L.kmws_unpack_gather(d_rows.data_ptr() + i * STRIDE, wl, d_hdr.data_ptr() + 16 * i, len(offs), mode,
                                  desc.data_ptr() + 64 * i, flags.data_ptr() + 64 * i, err.data_ptr() + 64 * i,
                                  dst.data_ptr() + SLOT * i, SLOT, doff.data_ptr() + 64 * i,
                                  ws.data_ptr() + gsz * i, gsz, None)
        assert st == 0, name
    T.cuda.synchronize()
    status = ws[:N * gsz].reshape(N, gsz)[:, :4].contiguous()
    _tail_check("kmws_unpack_gather", meta, want, desc[:N * 64], flags[:N * 64], err[:N * 64], status)
    got_dst = to_np(dst)[:N * SLOT].reshape(N, SLOT)
    got_off = to_np(doff)[:N * 64].view(np.int64).reshape(N, 8)
    for i, w in enumerate(want):
        name = meta[i][3]
        pay = b"".join(x[5] for x in w)
        lens = [x[2] for x in w]
        assert got_off[i, :len(w) + 1].tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist(), name
        assert np.all(got_off[i, len(w) + 1:] == -1), name
        assert got_dst[i, :len(pay)].tobytes() == pay and np.all(got_dst[i, len(pay):] == FILL), name
    assert np.array_equal(to_np(d_rows), flat)


# ------------------------------ the walks ------------------------------
_walk_cache = {}


def walk_want(stream, cap):
    key = (stream, cap)
    if key not in _walk_cache:
        _walk_cache[key] = hc.walk_expect(stream, cap)
    return _walk_cache[key]


def _ordered_streams():
    """The stream list with the cut streams last, so a batch built from it ends
    on a truncated header at the wire's end."""
    ws = hc.walk_streams()
    names = sorted(ws, key=lambda n: (n.startswith("cut_"), n))
    return [(n, ws[n]) for n in names]


def _check_walk(T, what, wire, off, streams, cap, slack):
    """One launch over a placed batch; every row against the oracle and the
    host walk.  slack 0: the wire ends with the last stream (its last headers
    are read byte by byte); slack 64: wire_len reaches 64 bytes further (0xFF
    bytes no stream covers), so every header goes through the aligned loads."""
    from kuma_amd import kmws
    ns = len(streams)
    assert off[-1] == len(wire) and len(off) == ns + 1
    base, d_wire = dev_wire(T, np.frombuffer(wire, np.uint8).copy(), slack=96)
    d_off = T.tensor(off, dtype=T.int64, device="cuda")
    hdr = T.full((ns, cap), -1, dtype=T.int64, device="cuda")
    got_hdr, n_out, used = kmws.find_headers_streams(d_wire, d_off, cap, wire_len=len(wire) + slack, hdr=hdr)
    T.cuda.synchronize()
    assert got_hdr.data_ptr() == hdr.data_ptr()
    got_hdr, n_out, used = to_np(got_hdr), to_np(n_out), to_np(used)
    for s, stream in enumerate(streams):
        offs, consumed = walk_want(stream, cap)
        tag = f"{what} cap {cap} slack {slack} stream {s} at {off[s]} ({len(stream)} bytes)"
        assert int(n_out[s]) == len(offs), tag
        assert (got_hdr[s, :len(offs)] - off[s]).tolist() == offs, tag
        assert np.all(got_hdr[s, len(offs):] == -1), tag  # untouched past n_out
        assert int(used[s]) == consumed, tag
        assert kmws.find_headers(stream, cap=cap) == (offs, consumed), tag  # host walk == device walk


def test_walk_streams_edges(T):
    named = _ordered_streams()
    caps = hc.WALK_CAPS
    # every stream at every start phase, in one batch (fillers between them; the
    # batch crosses the 256-lane block edge four times)
    items = [(s, ph) for ph in range(16) for _, s in named]
    wire, off, streams = hc.place_streams(items)
    assert len(streams) == 2 * len(items) - 1 > 1024
    for cap in caps:
        for slack in (0, 64):
            _check_walk(T, "all phases", wire, off, streams, cap, slack)
    # stream counts at the block edge; the start phases rotate with the position
    for ns in (255, 256, 257):
        items = [(named[(j + ns) % len(named)][1], (5 * j + ns) % 16) for j in range((ns + 1) // 2)]
        wire, off, streams = hc.place_streams(items, n_streams=ns)
        for cap in caps:
            for slack in (0, 64):
                _check_walk(T, f"{ns} streams", wire, off, streams, cap, slack)
    # one stream per launch, so each stream is the wire's last: at every phase
    # with one cap (rotating), the frame-count streams with every cap at two phases
    for j, (name, s) in enumerate(named):
        for ph in range(16):
            every = name.startswith("count_") and ph in (0, 9)
            wire, off, streams = hc.place_streams([(s, ph)], n_streams=1)
            for cap in (caps if every else [caps[(j + ph) % len(caps)]]):
                for slack in (0, 64):
                    _check_walk(T, name, wire, off, streams, cap, slack)
