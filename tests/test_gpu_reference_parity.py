"""The device paths against kuma's own compiled WSHandler.cpp.

Every expectation here comes from oracle/_ref/libkmws_ref_O3.so (the
reference's src/ws/WSHandler.cpp behind oracle/ref_wrap.cpp, built by
oracle/ref_build.py where the reference checkout is present; the built library
travels with the tree) -- never from oracle/kmws_oracle.c and never from the
checkout itself.  Skipped only where that library is absent.

  unmask     kmws_unmask_batch (default schedule) and kmws_gather_unmask against
             handleDataMask(key, data, len), frame by frame
  headers    kmws_unpack_headers / kmws_unpack_unmask / kmws_unpack_gather and
             kmws_find_headers_streams against decodeFrame (the corpus and the
             walk streams of tests/header_cases.py, expectations recomputed
             with the reference decoder)
  encode     kmws_encode_batch and kmws_pack_headers against encodeFrameHeader
             + handleDataMask, in the chunk form and in the unit form
  reframe    kmws_reframe_batch against decodeFrame followed by
             encodeFrameHeader + handleDataMask under the outgoing key
  decoder    kmws.WSHandler (resident worker on, off = launched) and RxBatch
             deferred + flush against the reference handler: return codes,
             callbacks, the caller's buffers, error / CLOSE / destroy sequences
  send       kmws_mask_host_chain and TxBatch against the KMBuffer-chain
             handleDataMask and encodeFrameHeader (sendWsFrame itself needs
             sockets and stays a restatement)
"""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import header_cases as hc  # noqa: E402
import pack_edge_cases as pec  # noqa: E402
import ref_cases as rc  # noqa: E402
from oracle import oracle as orc  # noqa: E402  (Hdr / Frame types and reference() only)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(orc.reference("O3") is None,
                                 reason="oracle/_ref/libkmws_ref_O3.so not built (the reference checkout was "
                                        "absent when build() ran)")]
FILL = 0xEE
SERVER, CLIENT = orc.SERVER, orc.CLIENT


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


@pytest.fixture(scope="module")
def R():
    return orc.reference("O3")


def to_np(t):
    return t.cpu().numpy()


def to_dev(T, a, slack=16):
    pad = (-len(a)) % 16
    return T.from_numpy(np.concatenate([np.asarray(a, np.uint8), np.zeros(pad + slack, np.uint8)])).cuda()


def first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return ("shapes", a.shape, b.shape)
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else int(d[0])


def key_bytes(k):
    return int(k).to_bytes(4, "little")


# ------------------------------ unmask vs handleDataMask ------------------------------
UNMASK_LENS = (0, 1, 3, 4, 15, 16, 17, 16383, 16384, 16385, 65531, 65536)


def _phase_batch():
    """Every length of UNMASK_LENS at every start offset mod 16 (192 frames),
    gaps of random bytes between them; every fifth key has a zero byte, every
    seventh is all zero."""
    rng = np.random.default_rng(0x554E4D31)
    offs, lens, cur = [], [], 0
    order = [(L, ph) for ph in range(16) for L in UNMASK_LENS]
    for i in rng.permutation(len(order)):
        L, ph = order[i]
        cur += (ph - cur) % 16 + (16 if rng.integers(0, 2) else 0)
        offs.append(cur)
        lens.append(L)
        cur += L
    keys = rng.integers(0, 2**32, size=len(offs), dtype=np.uint64).astype(np.uint32)
    keys[::5] &= np.uint32(0xFFFF00FF)
    keys[::7] = 0
    buf = rng.integers(0, 256, size=cur + 9, dtype=np.uint8)
    return buf, np.array(offs, np.int64), np.array(lens, np.int64), keys


def _tiny_batch():
    """700 frames of 1-40 bytes inside one 16 KiB tile (the general path)."""
    rng = np.random.default_rng(0x554E4D32)
    lens = rng.integers(1, 41, size=700)
    gaps = rng.integers(0, 3, size=700)
    starts = np.cumsum(np.concatenate([[0], gaps + lens]))
    offs = (starts[:-1] + gaps).astype(np.int64)
    total = int(starts[-1])
    assert total <= 16384
    keys = rng.integers(0, 2**32, size=700, dtype=np.uint64).astype(np.uint32)
    keys[::5] &= np.uint32(0xFF00FFFF)
    return rng.integers(0, 256, size=total, dtype=np.uint8), offs, lens.astype(np.int64), keys


@pytest.mark.parametrize("batch", [_phase_batch, _tiny_batch], ids=["every_phase", "tiny_one_tile"])
def test_unmask_kernels_vs_handle_data_mask(T, R, batch):
    from kuma_amd import kmws
    buf, offs, lens, keys = batch()
    want = buf.copy()
    for o, L, k in zip(offs, lens, keys):
        if L:
            R.mask(key_bytes(k), want[int(o):int(o) + int(L)], 0)  # a view: in place
    assert not np.array_equal(want, buf)
    n, span = len(offs), len(buf)
    descs = kmws.make_descs(offs, lens, keys.astype(np.int64))
    # in place
    d_buf = to_dev(T, buf, slack=0)
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    kmws.unmask_batch(d_buf, descs, ws, span)
    T.cuda.synchronize()
    assert ws.status() == 0
    got = to_np(d_buf)
    assert first_diff(got[:span], want) is None, ("kmws_unmask_batch: first wrong byte", first_diff(got[:span], want))
    assert not got[span:].any()
    # gather
    total = int(lens.sum())
    d_src = to_dev(T, buf)
    dst = T.full(((total + 64 + 15) // 16 * 16,), FILL, dtype=T.uint8, device="cuda")
    doff = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    wsg = kmws.Workspace(kmws.copy_workspace_size(n, dst.numel()))
    kmws.gather_unmask(d_src, descs, dst, doff, wsg)
    T.cuda.synchronize()
    assert wsg.status() == 0
    assert np.array_equal(to_np(doff), np.concatenate([[0], np.cumsum(lens)]))
    want_g = np.concatenate([want[int(o):int(o) + int(L)] for o, L in zip(offs, lens)])
    got_g = to_np(dst)
    assert first_diff(got_g[:total], want_g) is None, ("kmws_gather_unmask", first_diff(got_g[:total], want_g))
    assert np.all(got_g[total:] == FILL)
    assert np.array_equal(to_np(d_src)[:span], buf)


# ------------------------------ header parse vs decodeFrame ------------------------------
_expected = {}


def ref_expected(R, mode):
    """The corpus's expectations from the reference decoder (once per mode)."""
    if mode not in _expected:
        c = hc.corpus(mode)
        _expected[mode] = hc.Expected(c.wire, c.wire_len, c.hdr_off, mode, decoder=R.Decoder)
    return _expected[mode]


def _outputs(T, n):
    return (T.full((n, 2), -1, dtype=T.int64, device="cuda"), T.full((n,), -1, dtype=T.int16, device="cuda"),
            T.full((n,), 99, dtype=T.uint8, device="cuda"))


def _assert_frames(what, c, idx, desc, flags, err, e):
    got = np.concatenate([to_np(desc).reshape(-1, 2), (to_np(flags).astype(np.int64) & 0xFFFF).reshape(-1, 1),
                          to_np(err).astype(np.int64).reshape(-1, 1)], axis=1)
    want = np.concatenate([e.desc()[idx], e.flags[idx].reshape(-1, 1), e.err[idx].astype(np.int64).reshape(-1, 1)],
                          axis=1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        f = int(idx[bad[0]])
        kind = c.kinds[c.kind_id[f]] if c.kind_id[f] >= 0 else "tail"
        pytest.fail(f"{what}: {len(bad)} of {len(got)} frames differ; first is record {f} {kind} at "
                    f"{int(c.hdr_off[f])}: got {got[bad[0]].tolist()} want {want[bad[0]].tolist()}")


@pytest.mark.parametrize("mode", [SERVER, CLIENT], ids=["server", "client"])
def test_header_parse_vs_decode_frame(T, R, mode):
    from kuma_amd import kmws
    c, e = hc.corpus(mode), ref_expected(R, mode)
    W = c.wire_len
    size = (W + 64 + 31) // 16 * 16
    base = T.full((size,), 0xFF, dtype=T.uint8, device="cuda")
    base[:W] = T.from_numpy(c.wire).cuda()
    everything = np.arange(c.n)
    desc, flags, err = _outputs(T, c.n)
    ws = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
    kmws.unpack_headers(base, T.from_numpy(c.hdr_off).cuda(), mode, desc, flags, err, ws, wire_len=W)
    T.cuda.synchronize()
    _assert_frames("kmws_unpack_headers", c, everything, desc, flags, err, e)
    assert e.err.any() and (e.err == 0).any() and ws.status() == 2
    # the fused forms on the valid records
    good = np.nonzero(e.err == 0)[0]
    d_good = T.from_numpy(c.hdr_off[good]).cuda()
    want = to_np(base).copy()
    for f in good:
        if e.len[f]:
            want[e.off[f]:e.off[f] + e.len[f]] = np.frombuffer(e.payload[f], np.uint8)
    w = base.clone()
    desc, flags, err = _outputs(T, len(good))
    wsm = kmws.Workspace(kmws.unmask_workspace_size(W))
    kmws.unpack_unmask(w, d_good, mode, desc, flags, err, wsm, wire_len=W)
    T.cuda.synchronize()
    _assert_frames("kmws_unpack_unmask", c, good, desc, flags, err, e)
    assert wsm.status() == 0
    assert first_diff(to_np(w), want) is None, ("in-place decode: first wrong byte", first_diff(to_np(w), want))
    total = int(e.len[good].sum())
    dst = T.full(((total + 64 + 15) // 16 * 16,), FILL, dtype=T.uint8, device="cuda")
    doff = T.full((len(good) + 1,), -1, dtype=T.int64, device="cuda")
    desc, flags, err = _outputs(T, len(good))
    wsg = kmws.Workspace(kmws.copy_workspace_size(len(good), dst.numel()))
    kmws.unpack_gather(base, d_good, mode, desc, flags, err, dst, doff, wsg, wire_len=W)
    T.cuda.synchronize()
    _assert_frames("kmws_unpack_gather", c, good, desc, flags, err, e)
    assert wsg.status() == 0
    assert np.array_equal(to_np(doff), np.concatenate([[0], np.cumsum(e.len[good])]))
    got = to_np(dst)
    assert got[:total].tobytes() == b"".join(e.payload[f] for f in good)
    assert np.all(got[total:] == FILL)


def test_header_walk_vs_decode_frame(T, R):
    """kmws_find_headers_streams: every walk stream at every start phase in one
    batch, every cap, with the wire ending at the last stream and 64 bytes later."""
    from kuma_amd import kmws
    named = sorted(hc.walk_streams().items(), key=lambda kv: (kv[0].startswith("cut_"), kv[0]))
    items = [(s, ph) for ph in range(16) for _, s in named]
    wire, off, streams = hc.place_streams(items)
    ns = len(streams)
    cache = {}
    size = (len(wire) + 96 + 31) // 16 * 16
    d_wire = T.full((size,), 0xFF, dtype=T.uint8, device="cuda")
    d_wire[:len(wire)] = T.from_numpy(np.frombuffer(wire, np.uint8).copy()).cuda()
    d_off = T.tensor(off, dtype=T.int64, device="cuda")
    for cap in hc.WALK_CAPS:
        for slack in (0, 64):
            hdr = T.full((ns, cap), -1, dtype=T.int64, device="cuda")
            _, n_out, used = kmws.find_headers_streams(d_wire, d_off, cap, wire_len=len(wire) + slack, hdr=hdr)
            T.cuda.synchronize()
            g_hdr, g_n, g_used = to_np(hdr), to_np(n_out), to_np(used)
            for s, stream in enumerate(streams):
                if (stream, cap) not in cache:
                    cache[(stream, cap)] = hc.walk_expect(stream, cap, R.Decoder)
                offs, consumed = cache[(stream, cap)]
                tag = f"cap {cap} slack {slack} stream {s} at {off[s]} ({len(stream)} bytes)"
                assert int(g_n[s]) == len(offs), tag
                assert (g_hdr[s, :len(offs)] - off[s]).tolist() == offs, tag
                assert np.all(g_hdr[s, len(offs):] == -1), tag
                assert int(g_used[s]) == consumed, tag


# ------------------------------ encode vs encodeFrameHeader + mask ------------------------------
ENCODE_SMALL = tuple(L for L in rc.ENCODE_LENGTHS if L <= 127)            # 0, 1, 125, 126, 127
ENCODE_BIG = (65535, 65536, 65537, 70000)                                 # the table's lengths, capped at 70,000


def _encode_frames(seed, n):
    """n frames: each big length once masked and once unmasked, the others drawn
    from the small lengths (so the mean region stays below the chunk-form
    threshold and both forms can be selected by the capacity); any first byte."""
    rng = np.random.default_rng(seed)
    lens = [L for L in ENCODE_BIG for _ in (0, 1)]
    masks = [m for _ in ENCODE_BIG for m in (0, 1)]
    lens += list(rng.choice(ENCODE_SMALL, size=n - len(lens)))
    masks += list(rng.integers(0, 2, size=n - len(masks)))
    order = rng.permutation(n)
    lens, masks = np.array(lens, np.int64)[order], np.array(masks, np.int64)[order]
    b0 = rng.integers(0, 256, size=n)
    keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[::6] &= np.uint32(0x00FFFFFF)
    flags = (b0 | (masks << 8)).astype(np.uint32)
    src, offs, _ = pec.layout_source(f"refenc-{seed}", lens)
    return src, offs, lens, flags, keys


def _cap_for(form, n, total):
    cap = total + 5000 if form == "chunks" else max(total, pec.kChunkFormBelow * n) + 777
    assert pec.use_chunks(n, cap) == (form == "chunks"), (form, n, cap)
    return cap


def test_encode_vs_encode_frame_header(T, R):
    from kuma_amd import kmws
    n = 300
    src, offs, lens, flags, keys = _encode_frames(0x454E4331, n)
    frames = [rc.wire_frame(R, int(fl) & 0xFF, (int(fl) >> 8) & 1, int(L), key_bytes(k),
                            src[int(o):int(o) + int(L)].tobytes())
              for o, L, fl, k in zip(offs, lens, flags, keys)]
    hls = [len(f) - int(L) for f, L in zip(frames, lens)]
    want = np.frombuffer(b"".join(frames), np.uint8)
    want_off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
    total = len(want)
    d_src = to_dev(T, src)
    descs = kmws.make_descs(offs.astype(np.int64), lens, keys.astype(np.int64))
    d_fl = T.from_numpy(flags.astype(np.int16)).cuda()
    for form in ("chunks", "units"):
        cap = _cap_for(form, n, total)
        dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        ws = kmws.Workspace(kmws.copy_workspace_size(n, cap))
        kmws.encode_batch(d_src, descs, d_fl, dst, off, ws)
        T.cuda.synchronize()
        assert ws.status() == 0, form
        assert np.array_equal(to_np(off), want_off), form
        got = to_np(dst)
        assert first_diff(got[:total], want) is None, (form, "first wrong byte", first_diff(got[:total], want))
        assert np.all(got[total:] == FILL), form
    # headers only: 16-byte slots, zero-padded
    hdr = T.full((16 * n,), FILL, dtype=T.uint8, device="cuda")
    hl = T.full((n,), 99, dtype=T.uint8, device="cuda")
    woff = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
    wsp = kmws.Workspace(kmws.pack_headers_workspace_size(n))
    kmws.pack_headers(descs, d_fl, hdr, hl, woff, wsp)
    T.cuda.synchronize()
    assert wsp.status() == 0
    slots = np.zeros((n, 16), np.uint8)
    for i, (f, h) in enumerate(zip(frames, hls)):
        slots[i, :h] = np.frombuffer(f[:h], np.uint8)
    assert np.array_equal(to_np(hdr).reshape(n, 16), slots)
    assert to_np(hl).tolist() == hls
    assert np.array_equal(to_np(woff), want_off)


# ------------------------------ reframe ------------------------------
def _plain_header(b0, mask, L, key):
    m = 0x80 if mask else 0
    if L <= 125:
        h = bytes([b0, m | L])
    elif L <= 0xFFFF:
        h = bytes([b0, m | 126]) + L.to_bytes(2, "big")
    else:
        h = bytes([b0, m | 127]) + L.to_bytes(8, "big")
    return h + (key if mask else b"")


def _xor(key, data):
    a = np.frombuffer(data, np.uint8)
    return (a ^ np.resize(np.frombuffer(key, np.uint8), len(a))).tobytes() if len(a) else b""


def test_reframe_vs_decode_then_encode(T, R):
    """64 masked frames in, re-encoded under outgoing flags and keys: the
    reference decodes the incoming wire (its callbacks give the descriptors and
    the plain payloads) and encodes the outgoing one."""
    from kuma_amd import kmws
    rng = np.random.default_rng(0x52454631)
    n = 64
    lens = [65535, 65536, 70000] + list(rng.choice([0, 1, 5, 125, 126, 127, 300, 4096], size=n - 3))
    lens = [int(lens[i]) for i in rng.permutation(n)]
    wire = b""
    for L in lens:
        key = bytes(rng.integers(0, 256, size=4, dtype=np.uint8))
        b0 = int(rng.choice([0x81, 0x82, 0x02, 0x01, 0x80, 0x00]))
        wire += _plain_header(b0, 1, L, key) + _xor(key, rng.integers(0, 256, size=L, dtype=np.uint8).tobytes())
    rets, fr = R.decode_chunks(wire, SERVER, 0)
    assert rets == [0] and len(fr) == n and [f.length for f in fr] == lens
    offs, p = [], 0
    for f in fr:
        p += rc.hdr_len(f.length, f.mask)
        offs.append(p)
        p += f.length
    in_keys = np.array([int.from_bytes(f.maskey, "little") for f in fr], np.int64)
    out_b0 = rng.integers(0, 256, size=n)
    out_mask = rng.integers(0, 2, size=n)
    out_keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    out_keys[::5] &= np.uint32(0xFF00FFFF)
    frames = [rc.wire_frame(R, int(b), int(m), f.length, key_bytes(k) if m else bytes(4), f.payload)
              for b, m, k, f in zip(out_b0, out_mask, out_keys, fr)]
    want = np.frombuffer(b"".join(frames), np.uint8)
    want_off = np.concatenate([[0], np.cumsum([len(x) for x in frames])]).astype(np.int64)
    total = len(want)
    d_src = to_dev(T, np.frombuffer(wire, np.uint8))
    descs = kmws.make_descs(np.array(offs, np.int64), np.array(lens, np.int64), in_keys)
    d_fl = T.from_numpy((out_b0 | (out_mask << 8)).astype(np.int16)).cuda()
    d_ok = T.from_numpy(out_keys.view(np.int32)).cuda()
    for form in ("chunks", "units"):
        cap = _cap_for(form, n, total)
        dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        ws = kmws.Workspace(kmws.reframe_workspace_size(n, cap))
        kmws.reframe_batch(d_src, descs, d_fl, d_ok, dst, off, ws)
        T.cuda.synchronize()
        assert ws.status() == 0, form
        assert np.array_equal(to_np(off), want_off), form
        got = to_np(dst)
        assert first_diff(got[:total], want) is None, (form, "first wrong byte", first_diff(got[:total], want))
        assert np.all(got[total:] == FILL), form
    assert to_np(d_src)[:len(wire)].tobytes() == wire


# ------------------------------ streaming decoder ------------------------------
SMALL_SIZES = (0, 1, 3, 5, 17, 125, 126, 127, 300)
BIG_SIZES = SMALL_SIZES + (4096, 16385, 65535, 65536)
CHUNKS = (1, 7, 4096, 0)


def _frames_40(seed, sizes, mode):
    """40 frames a decoder in `mode` accepts, built in plain Python."""
    rng = random.Random(seed)
    out = []
    for _ in range(40):
        op = rng.choice([0, 1, 2, 2, 9, 10, 3])
        L = rng.choice(sizes)
        if op >= 8:
            L = min(L, 125)
        fin = 1 if op >= 8 else rng.randrange(2)
        b0 = (fin << 7) | (rng.randrange(8) << 4 if rng.random() < 0.3 else 0) | op
        key = bytes(rng.randrange(256) for _ in range(4))
        mask = 1 if mode == SERVER else 0
        payload = rng.randbytes(L)
        out.append(_plain_header(b0, mask, L, key) + (_xor(key, payload) if mask else payload))
    return out


def _streams(chunk):
    """{name: (mode, stream, destroy_on)} for one chunk size: the small sizes for
    the byte-sized chunks, frames up to 64 KiB for the others."""
    sizes = SMALL_SIZES if chunk in (1, 7) else BIG_SIZES
    seed = 4000 + chunk
    fr = _frames_40(seed, sizes, SERVER)
    close = _plain_header(0x88, 1, 2, b"\x0a\x0b\x0c\x0d") + _xor(b"\x0a\x0b\x0c\x0d", b"\x03\xe8")
    out = {
        "valid": (SERVER, b"".join(fr), None),
        "valid_client": (CLIENT, b"".join(_frames_40(seed + 1, sizes, CLIENT)), None),
        "unmasked_frame_in_the_middle": (SERVER, b"".join(fr[:20]) + b"\x82\x03abc" + b"".join(fr[20:]), None),
        "length_error_in_the_middle": (SERVER, b"".join(fr[:20]) + b"\x82\xfe\x00\x7d" + b"".join(fr[20:]), None),
        "close_in_the_middle": (SERVER, b"".join(fr[:20]) + close + b"".join(fr[20:]), None),
        "destroy_at_15": (SERVER, b"".join(fr), 15),
        "destroy_at_close": (SERVER, b"".join(fr[:20]) + close + b"".join(fr[20:]), 20),
    }
    return out


def _hdr_key(hd, p):
    return (hd.fin, hd.rsv1, hd.rsv2, hd.rsv3, hd.opcode, hd.mask, hd.plen, hd.xpl64, bytes(hd.maskey), hd.length, p)


def _run_sync(mode, stream, chunk, destroy_on):
    from kuma_amd import kmws
    h = kmws.WSHandler(mode)
    got = []

    def cb(hd, p):
        got.append(_hdr_key(hd, p))
        return destroy_on is not None and len(got) - 1 == destroy_on

    h.setFrameCallback(cb)
    rets, counts, bufs = [], [], []
    step = chunk if chunk > 0 else max(1, len(stream))
    for i in range(0, len(stream), step):
        piece = bytearray(stream[i:i + step])
        ret = h.handleData(piece)
        rets.append(ret)
        counts.append(len(got))
        bufs.append(bytes(piece))
        if ret == rc.DESTROYED:
            break
    return rets, counts, bufs, got


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}" if c else "whole")
def test_sync_decoder_vs_reference_handler(T, R, chunk, resident):
    from kuma_amd import kmws
    if not resident:
        kmws.resident_enable(False)
    try:
        for name, (mode, stream, destroy_on) in _streams(chunk).items():
            want = rc.run_stream(R, mode, stream, chunk, destroy_on)
            rets, counts, bufs, got = _run_sync(mode, stream, chunk, destroy_on)
            assert rets == want.rets, (name, "return codes")
            assert counts == want.counts, (name, "callback counts")
            assert got == want.frames, (name, "callbacks")
            assert bufs == want.buffers, (name, "caller's buffers")
    finally:
        if not resident:
            kmws.resident_enable(True)


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk{c}" if c else "whole")
def test_deferred_decoder_vs_reference_handler(T, R, chunk):
    """RxBatch: feeds parse and return at once, callbacks arrive at flush.  The
    return codes of every feed and the callbacks are the reference's; where the
    callback destroys the handler, delivery stops with that frame and the
    handler is not fed again (the feeds of that flush had been parsed before,
    so their return codes are not compared)."""
    from kuma_amd import kmws
    for name, (mode, stream, destroy_on) in _streams(chunk).items():
        want = rc.run_stream(R, mode, stream, chunk, destroy_on)
        batch = kmws.RxBatch(0)
        h = kmws.WSHandler(mode)
        got = []

        dead = []

        def cb(hd, p):
            got.append(_hdr_key(hd, p))
            if destroy_on is not None and len(got) - 1 == destroy_on:
                dead.append(True)
            return bool(dead)

        h.setFrameCallback(cb)
        rets = []
        step = chunk if chunk > 0 else max(1, len(stream))
        for k, i in enumerate(range(0, len(stream), step)):
            rets.append(h.handleDataDeferred(batch, stream[i:i + step]))
            if k % 64 == 63:
                batch.flush()
                if dead:
                    break  # the handler is gone: it is not fed again
        batch.flush()
        assert batch.pending() == 0
        assert got == want.frames, (name, "callbacks")
        if destroy_on is None:
            assert rets == want.rets, (name, "return codes")


# ------------------------------ send path ------------------------------
SEND_SIZES = (0, 1, 3, 5, 4096, 65536)


def _chains():
    rng = random.Random(0x53454E44)
    out = []
    for nseg in range(1, 8):
        for rep in range(4):
            sizes = [rng.choice(SEND_SIZES) for _ in range(nseg)]
            if rep == 0:
                sizes[rng.randrange(nseg)] = 0
            if rep == 1 and nseg > 1:
                sizes[0] = 0
                sizes[-1] = 5
            key = bytes(rng.randrange(256) for _ in range(4))
            if rep == 2:
                key = key[:2] + b"\0" + key[3:]
            out.append((key, [rng.randbytes(s) for s in sizes]))
    return out


def test_mask_host_chain_vs_kmbuffer_chain_mask(T, R):
    from kuma_amd import kmws
    for key, segs in _chains():
        want = R.mask_chain(key, segs)
        mine = [bytearray(s) for s in segs]
        kmws.handle_data_mask(key, mine)
        assert [bytes(x) for x in mine] == want, (key.hex(), [len(s) for s in segs])


def test_tx_batch_vs_encode_frame_header_and_chain_mask(T, R):
    from kuma_amd import kmws
    rng = random.Random(0x54584231)
    b = kmws.TxBatch()
    sends, want = [], []
    for i, (key, segs) in enumerate(_chains()):
        mask = 0 if i % 5 == 4 else 1
        b0 = rng.randrange(256)
        hdr = kmws.Header(fin=b0 >> 7, rsv1=(b0 >> 6) & 1, rsv2=(b0 >> 5) & 1, rsv3=(b0 >> 4) & 1, opcode=b0 & 15,
                          mask=mask, maskey=key)
        plen = sum(len(s) for s in segs)
        wh = R.encode_header(orc.Hdr(fin=hdr.fin, rsv1=hdr.rsv1, rsv2=hdr.rsv2, rsv3=hdr.rsv3, opcode=hdr.opcode,
                                     mask=mask, maskey=key, length=plen))
        want.append((wh, R.mask_chain(key, segs) if mask else [bytes(s) for s in segs]))
        sends.append((hdr, [bytearray(s) for s in segs]))
    got_hdrs = [b.add(h, segs) for h, segs in sends]
    assert got_hdrs == [w[0] for w in want]
    queued = sum(1 for h, segs in sends if h.mask and sum(map(len, segs)))
    assert b.pending() == queued
    assert b.flush() == queued
    for i, ((h, segs), (wh, wsegs)) in enumerate(zip(sends, want)):
        assert [bytes(x) for x in segs] == wsegs, i
