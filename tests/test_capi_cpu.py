"""C-ABI checks that need no GPU: the library loads and exports every symbol
include/kmws_gpu.h and include/kmws_bench.h declare; host codec entries match
the oracle."""
import os
import random
import re

import pytest

from kuma_amd import kmws
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_decls(name="kmws_gpu.h"):
    txt = open(os.path.join(ROOT, "include", name)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(kmws_[a-z0-9_]+)\s*\(", txt))
    return sorted(n for n in names if n != "kmws_make_flags")  # static inline helper


def test_exports_every_declared_symbol():
    L = kmws.lib()
    decl = header_decls()
    assert len(decl) >= 15
    for name in decl:
        assert hasattr(L, name), name
    assert sorted(kmws.EXPORTS) == decl
    bench = header_decls("kmws_bench.h")
    for name in bench:
        assert hasattr(L, name), name
    assert sorted(kmws.BENCH_EXPORTS) == bench


def test_public_header_has_no_tuning_entries():
    """The drop-in header carries only boundary entries: no tuning variants,
    no device-global schedule query, no persistent-grid probes."""
    decl = header_decls()
    for gone in ("kmws_unmask_batch_variant", "kmws_unmask_schedule", "kmws_unmask_resident_blocks",
                 "kmws_arena_alloc", "kmws_fill_synthetic"):
        assert gone not in decl
    L = kmws.lib()
    assert not hasattr(L, "kmws_unmask_batch_variant") and not hasattr(L, "kmws_unmask_resident_blocks")


def test_encode_header_matches_oracle():
    rng = random.Random(7)
    lens = [0, 1, 2, 124, 125, 126, 127, 65534, 65535, 65536, 65537, 10485760, 2**31, 2**32 - 1]
    lens += [rng.randrange(2**32) for _ in range(200)]
    for L in lens:
        for mask in (0, 1):
            h = dict(fin=rng.randrange(2), rsv1=rng.randrange(2), rsv2=rng.randrange(2),
                     rsv3=rng.randrange(2), opcode=rng.randrange(16), mask=mask,
                     maskey=bytes(rng.randrange(256) for _ in range(4)), length=L)
            got = kmws.encode_frame_header(kmws.Header(**h))
            assert got == orc.encode_header(orc.Hdr(**h))
            assert len(got) == kmws.header_size(L, mask)


def _client_stream(rng, nframes):
    out = b""
    for _ in range(nframes):
        n = rng.choice([0, 1, 3, 125, 126, 200, 65535, 65536, 70001])
        op = rng.choice([0, 1, 2, 3, 9, 10])
        h = orc.Hdr(fin=1 if op >= 8 else rng.randrange(2), opcode=op, mask=0,
                    length=min(n, 125) if op >= 8 else n)
        out += orc.encode_header(h) + bytes(rng.randrange(256) for _ in range(h.length))
    return out


@pytest.mark.parametrize("chunk", [0, 1, 5, 64, 1000, 65536])
def test_decoder_unmasked_matches_oracle(chunk):
    """CLIENT-mode streams carry no masked payload, so no device work is needed."""
    rng = random.Random(100 + chunk)
    stream = _client_stream(rng, 12 if chunk == 1 else 60)
    rets_o, frames_o = orc.decode_chunks(stream, orc.CLIENT, chunk)
    h = kmws.WSHandler(kmws.CLIENT)
    got = []
    h.setFrameCallback(lambda hd, p: got.append((hd.fin, hd.rsv1, hd.rsv2, hd.rsv3, hd.opcode, hd.mask,
                                                 hd.plen, hd.xpl64, hd.maskey, hd.length, p)))
    rets = []
    if chunk <= 0:
        rets.append(h.handleData(stream))
    else:
        for i in range(0, len(stream), chunk):
            rets.append(h.handleData(stream[i:i + chunk]))
    assert rets == rets_o
    assert got == [f.key() for f in frames_o]


def test_decoder_golden_client_cases():
    import json
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_vectors.json")))
    ran = 0
    for c in gold["decode"]:
        if c["mode"] != "CLIENT":
            continue
        data = bytes.fromhex(c["input_hex"])
        if "tail_gen" in c:
            data += bytes(c["tail_len"]) if c["tail_gen"] == "zeros" else \
                bytes(i & 0xFF for i in range(c["tail_len"]))
        h = kmws.WSHandler(kmws.CLIENT)
        frames = []
        h.setFrameCallback(lambda hd, p: frames.append((hd, p)))
        step = c["chunk"] or len(data) or 1
        rets = [h.handleData(data[i:i + step]) for i in range(0, max(1, len(data)), step)]
        assert rets == c["expect_rets"], c["name"]
        assert len(frames) == len(c["expect_frames"]), c["name"]
        for (hd, p), e in zip(frames, c["expect_frames"]):
            assert (hd.fin, hd.opcode, hd.mask, hd.length) == (e["fin"], e["opcode"], e["mask"], e["length"])
        for s in c.get("then", []):
            assert h.handleData(bytes.fromhex(s["input_hex"])) == s["expect_rets"][0]
        ran += 1
    assert ran >= 15


def test_masked_frame_without_gpu_fails_loudly():
    if kmws.device_count() > 0:
        pytest.skip("GPU present")
    h = kmws.WSHandler(kmws.SERVER)
    assert h.handleData(bytes.fromhex("818537fa213d7f9f4d5158")) == kmws.ERR_NOT_SUPPORTED


def test_synthetic_host_generator():
    a = orc.synthetic(5, 0, 64)
    b = orc.synthetic(5, 13, 40)
    assert (a[13:53] == b).all()
    w = orc.splitmix64(5 + 1).to_bytes(8, "little")
    assert bytes(a[8:16]) == w


def test_find_headers_matches_oracle_walk():
    rng = random.Random(21)
    stream, offs = b"", []
    for _ in range(200):
        n = rng.choice([0, 1, 125, 126, 65535, 65536, 70000])
        h = orc.encode_header(orc.Hdr(opcode=rng.choice([0, 1, 2]), mask=rng.randrange(2),
                                      maskey=b"abcd", length=n))
        offs.append(len(stream))
        stream += h + bytes(n)
    got, used = kmws.find_headers(stream)
    assert got == offs and used == len(stream)
    # truncated tail: last frame recorded, consumed stops before it
    got, used = kmws.find_headers(stream[:-1])
    assert got == offs and used == offs[-1]
    # CLOSE stops the walk (WSHandler.cpp:265-268)
    close = orc.encode_header(orc.Hdr(opcode=8, length=0))
    got, used = kmws.find_headers(close + stream)
    assert got == [0] and used == 2
    # invalid 127-class length is recorded and ends the walk
    got, _ = kmws.find_headers(bytes.fromhex("827f4000000000000000") + stream)
    assert got == [0]


def test_arena_alloc_without_device_returns_null():
    """No gfx950 device here: kmws_arena_alloc reports failure (NULL), no crash."""
    import ctypes as C
    from kuma_amd import kmws
    if kmws.lib().kmws_device_count() > 0:
        pytest.skip("a device is present")
    flag = C.c_int(7)
    assert not kmws.lib().kmws_arena_alloc(1 << 20, 0, C.byref(flag))
    assert flag.value == 0
    kmws.lib().kmws_arena_free(None, 0)


def test_tx_batch_without_device_is_null():
    """No gfx950 device here: kmws_tx_batch_create returns NULL (no CPU fallback)."""
    from kuma_amd import kmws
    if kmws.lib().kmws_device_count() > 0:
        pytest.skip("a device is present")
    assert not kmws.lib().kmws_tx_batch_create(0)
    with pytest.raises(RuntimeError):
        kmws.TxBatch()


def test_batch_entries_reject_bad_arguments_before_any_device_work():
    """Argument checks of the device batch entries return kuma's INVALID_PARAM /
    BUFFER_TOO_SMALL without launching anything (so they hold with no GPU)."""
    import ctypes as C
    L = kmws.lib()
    fake = C.c_void_p(16)      # never dereferenced: every call below fails its checks first
    odd = C.c_void_p(16 + 8)   # not 16-byte aligned
    assert L.kmws_pack_headers(None, None, 5, fake, None, None, None, 0, None) == kmws.ERR_INVALID_PARAM
    assert L.kmws_pack_headers(fake, fake, 5, odd, None, None, None, 0, None) == kmws.ERR_INVALID_PARAM
    assert L.kmws_pack_headers(fake, fake, 5, fake, None, fake, None, 0, None) == kmws.ERR_INVALID_PARAM
    need = L.kmws_pack_headers_workspace_size(5)
    assert need >= 16
    assert L.kmws_pack_headers(fake, fake, 5, fake, None, fake, fake, need - 1, None) == kmws.ERR_BUFFER_TOO_SMALL
    assert L.kmws_find_headers_streams(fake, 64, None, 3, fake, 4, fake, None, None) == kmws.ERR_INVALID_PARAM
    assert L.kmws_find_headers_streams(fake, 64, fake, 3, None, 4, fake, None, None) == kmws.ERR_INVALID_PARAM
    assert L.kmws_find_headers_streams(None, 0, None, 0, None, 0, None, None, None) == 0  # nothing to do


def _copy_entry_rows():
    """(entry, argument list, expected status) for the five copy entries the
    reframe's table (test_reframe_capi_cpu.py) does not cover.  Pointers are
    fakes that are never dereferenced: every row fails its checks."""
    import ctypes as C
    L = kmws.lib()
    n, cap, S = 5, 1 << 16, kmws.SERVER
    fake, odd = C.c_void_p(4096), C.c_void_p(4096 + 8)
    bad, small = kmws.ERR_INVALID_PARAM, kmws.ERR_BUFFER_TOO_SMALL
    need = L.kmws_copy_workspace_size(n, cap)
    need8 = L.kmws_gather_utf8_workspace_size(n, cap, 1)
    need0 = L.kmws_gather_utf8_workspace_size(0, cap, 1)
    # name: (valid call, index of n, of workspace and of workspace_bytes, required pointers, aligned pointers,
    #        index of mode or None, sufficient size)
    entries = {
        #                     src   descs flags n  dst   cap  off   ws    bytes stream
        "kmws_encode_batch": ([fake, fake, fake, n, fake, cap, fake, fake, need, None],
                              3, 7, 8, (0, 1, 2, 4, 6, 7), (0, 4), None),
        #                      src   descs n  dst   cap  off   ws    bytes stream
        "kmws_gather_unmask": ([fake, fake, n, fake, cap, fake, fake, need, None],
                               2, 6, 7, (0, 1, 3, 5, 6), (0, 3), None),
        #                      wire  len      hdr   n  mode desc  flags err   dst   cap  off   ws    bytes stream
        "kmws_unpack_gather": ([fake, 1 << 16, fake, n, S, fake, fake, fake, fake, cap, fake, fake, need, None],
                               3, 11, 12, (0, 2, 5, 8, 10, 11), (0, 8), 4),
        #                           src   descs flags n  dst   cap  off   first ns carry      utf8  ws    bytes stream
        "kmws_gather_unmask_utf8": ([fake, fake, fake, n, fake, cap, fake, None, 1, None, None, fake, fake, need8, None],
                                    3, 12, 13, (0, 1, 2, 4, 6, 11, 12), (0, 4), None),
        #                           wire  len      hdr   n  mode desc  flags err   dst   cap  off   first ns carry
        "kmws_unpack_gather_utf8": ([fake, 1 << 16, fake, n, S, fake, fake, fake, fake, cap, fake, None, 1, None, None,
                                     fake, fake, need8, None],  # out_utf8, workspace, bytes, stream
                                    3, 16, 17, (0, 2, 5, 6, 8, 10, 15, 16), (0, 8), 4),
    }
    rows = []

    def row(name, ok, want, **changes):
        args = list(ok)
        for i, v in changes.items():
            args[int(i[1:])] = v
        rows.append((name, args, want))

    for name, (ok, i_n, i_ws, i_sz, required, aligned, i_mode) in entries.items():
        plain = not name.endswith("_utf8")
        full = ok[i_sz]
        for i in required:  # each required pointer NULL in turn (the workspace among them: NULL, sufficient size)
            row(name, ok, bad, **{f"a{i}": None})
        for i in aligned:  # 16-byte alignment of the source and of dst
            row(name, ok, bad, **{f"a{i}": odd})
        row(name, ok, small, **{f"a{i_sz}": full - 1})
        row(name, ok, small, **{f"a{i_sz}": 0})
        # a NULL workspace is a bad argument whatever size goes with it
        row(name, ok, bad, **{f"a{i_ws}": None, f"a{i_sz}": full - 1})
        if i_mode is not None:
            for m in (7, -1):
                row(name, ok, bad, **{f"a{i_mode}": m})
        if plain:
            # with a workspace that is there and too small, that is what any failing call reports
            row(name, ok, small, a0=None, **{f"a{i_sz}": full - 1})
            row(name, ok, small, a0=odd, **{f"a{i_sz}": full - 1})
            if i_mode is not None:
                row(name, ok, small, **{f"a{i_mode}": 7, f"a{i_sz}": full - 1})
        else:
            # utf8_stream_args_check's order: counts, pointers, alignment, streams, then the size
            row(name, ok, bad, a0=None, **{f"a{i_sz}": full - 1})
            row(name, ok, bad, a0=odd, **{f"a{i_sz}": full - 1})
            row(name, ok, bad, **{f"a{i_n}": 1 << 31})
            i_first = i_ws - 5  # stream_first, then n_streams
            row(name, ok, bad, **{f"a{i_first + 1}": 0})
            row(name, ok, bad, **{f"a{i_first + 1}": 2})  # several streams need stream_first
            row(name, ok, bad, **{f"a{i_first + 1}": 1 << 31, f"a{i_first}": fake})
            row(name, ok, bad, **{f"a{i_first + 1}": 0, f"a{i_sz}": 0})
            if i_mode is not None:  # the mode comes before everything else
                row(name, ok, bad, **{f"a{i_mode}": 7, f"a{i_sz}": 0})
        # an empty batch with NULL data pointers still needs its offsets array and its workspace
        empty = [None if isinstance(v, C.c_void_p) else v for v in ok]
        empty[i_n] = 0
        i_off = i_ws - 1 if plain else i_ws - 6
        size0 = L.kmws_copy_workspace_size(0, cap) if plain else need0
        row(name, empty, bad, **{f"a{i_ws}": fake, f"a{i_sz}": size0})               # offsets NULL
        row(name, empty, bad, **{f"a{i_off}": fake, f"a{i_sz}": size0})              # workspace NULL
        row(name, empty, small, **{f"a{i_off}": fake, f"a{i_ws}": fake, f"a{i_sz}": size0 - 1})
        if plain:
            row(name, empty, bad, **{f"a{i_off}": fake, f"a{i_sz}": size0 - 1})      # NULL and short: still a bad argument
        else:
            row(name, empty, bad, a0=odd, **{f"a{i_off}": fake, f"a{i_ws}": fake, f"a{i_sz}": size0})
    return rows


def test_copy_entries_reject_bad_arguments_before_any_device_work():
    """The status every copy entry returns for each bad argument, and which check
    wins when two fail: kmws_encode_batch, kmws_gather_unmask and
    kmws_unpack_gather report BUFFER_TOO_SMALL only for a workspace that is there
    and too small (then whatever else is wrong), otherwise INVALID_PARAM; the
    UTF-8 gathers check their mode, then follow kmws_utf8_validate's order, the
    size last.  No row reaches a launch, so the table holds with and without a
    device."""
    L = kmws.lib()
    rows = _copy_entry_rows()
    assert len(rows) >= 100 and len({r[0] for r in rows}) == 5
    got = [(name, i, getattr(L, name)(*args)) for i, (name, args, _) in enumerate(rows)]
    assert got == [(name, i, want) for i, (name, _, want) in enumerate(rows)]


def test_batch_entries_with_a_null_handle():
    """The status of every rx / tx batch entry and of kmws_decoder_feed_deferred
    for a NULL handle, and of kmws_tx_batch_poll for a negative ticket.  The two
    attach entries differ (rx: INVALID_STATE, tx: INVALID_PARAM).  No row
    dereferences a handle, so the table holds with and without a device."""
    import ctypes as C
    L = kmws.lib()
    bad, state = kmws.ERR_INVALID_PARAM, kmws.ERR_INVALID_STATE
    fake = C.c_void_p(4096)  # never dereferenced: the rows that pass it fail on another argument first
    hdr = kmws.Header(fin=1, opcode=2, mask=1, maskey=b"abcd").to_c()
    seg = (C.c_uint8 * 4)()
    segs, lens = (C.c_void_p * 1)(C.addressof(seg)), (C.c_size_t * 1)(4)
    out = (C.c_uint8 * kmws.MAX_HEADER_SIZE)()
    cb = kmws.FRAME_CB(lambda hp, p, n, u: 0)
    dec = L.kmws_decoder_create(kmws.SERVER, 0)
    assert dec
    rows = [
        ("kmws_rx_batch_pending", [None], 0),
        ("kmws_rx_batch_pending_bytes", [None], 0),
        ("kmws_rx_batch_inflight", [None], 0),
        ("kmws_rx_batch_submit", [None], bad),
        ("kmws_rx_batch_poll", [None, 0], bad),
        ("kmws_rx_batch_poll", [None, 1], bad),
        ("kmws_rx_batch_flush", [None], bad),
        ("kmws_rx_batch_attach_ring", [None, None, 0], state),
        ("kmws_rx_batch_attach_ring", [None, fake, 4096], state),
        ("kmws_rx_batch_discard", [None, None], None),
        ("kmws_rx_batch_discard", [None, dec], None),
        ("kmws_rx_batch_destroy", [None], None),
        ("kmws_tx_batch_pending", [None], 0),
        ("kmws_tx_batch_submit", [None], bad),
        ("kmws_tx_batch_poll", [None, 0, 0], bad),
        ("kmws_tx_batch_poll", [None, 1, 1], bad),
        ("kmws_tx_batch_poll", [None, -1, 0], bad),
        ("kmws_tx_batch_poll", [fake, -1, 0], bad),
        ("kmws_tx_batch_poll", [fake, -(1 << 62), 1], bad),
        ("kmws_tx_batch_flush", [None], bad),
        ("kmws_tx_batch_add", [None, C.byref(hdr), segs, lens, 1, out], bad),
        ("kmws_tx_batch_attach_ring", [None, None, 0], bad),
        ("kmws_tx_batch_attach_ring", [None, fake, 4096], bad),
        ("kmws_tx_batch_destroy", [None], None),
        ("kmws_decoder_feed_deferred", [None, None, seg, 4, cb, None], bad),
        ("kmws_decoder_feed_deferred", [None, fake, seg, 4, cb, None], bad),
        ("kmws_decoder_feed_deferred", [dec, None, seg, 4, cb, None], bad),
        ("kmws_decoder_feed_deferred", [dec, None, None, 0, cb, None], bad),
        ("kmws_decoder_feed_deferred", [dec, fake, None, 4, cb, None], bad),  # data NULL with a length
    ]
    try:
        got = [(name, i, getattr(L, name)(*args)) for i, (name, args, _) in enumerate(rows)]
    finally:
        L.kmws_decoder_destroy(dec)
    assert got == [(name, i, want) for i, (name, _, want) in enumerate(rows)]
    every = {n for n in kmws.EXPORTS if n.startswith(("kmws_rx_batch_", "kmws_tx_batch_"))}
    assert every - {r[0] for r in rows} == {"kmws_rx_batch_create", "kmws_tx_batch_create"}


def test_copy_workspace_size_follows_the_copy_form():
    """kmws_copy_workspace_size (no device needed): below a 16 KiB mean region
    bound (dst_cap / n) the chunk form's 8 B per 4 KiB output chunk, from it the
    unit form's edge words (80 B per frame) and 32-byte unit records -- so the
    same (n, dst_cap) the call passes must size the workspace."""
    n = 1000
    small = kmws.copy_workspace_size(n, n * 4104)        # cfg4-like: chunk form
    large = kmws.copy_workspace_size(n, n * 65550)       # 64 KiB frames: unit form
    chunks = -(-n * 4104 // 4096)
    assert small >= 8 * chunks and small < 8 * chunks + 64 * 1024
    assert large >= 80 * n + 32 * (n * 65550 // 4096)
    # the threshold: dst_cap / n crosses 16 KiB
    below = kmws.copy_workspace_size(n, n * 16383)
    above = kmws.copy_workspace_size(n, n * 16384)
    assert above > below + 80 * n // 2
    assert kmws.copy_workspace_size(0, 0) > 0


def test_device_batch_busy_without_batches():
    """kmws_device_batch_busy (no device needed): 0 before any device batch was
    enqueued, and for devices out of range."""
    L = kmws.lib()
    assert [L.kmws_device_batch_busy(d) for d in (0, 1, -1, 64, 1 << 20)] == [0, 0, 0, 0, 0]
    assert kmws.device_batch_busy(0) is False
