"""The receive loop of a device-batch server, run
three ways over one corpus of connections whose TCP reads cut frames anywhere:

  handler_loop  a kmws.WSHandler per connection, fed read by read (the drop-in);
  device_loop   the connections' reads of one round back to back in one wire,
                through kmws_find_headers_streams, one kmws_unpack_* payload
                pass, kmws_proto_check, and two carries per connection;
  model_loop    the same bookkeeping on the host alone: the host walk
                (kmws.find_headers) and a header parse written here from the
                decoder's state order -- no GPU, so the CPU suite pins it.

Nothing here touches the GPU at import.  The references are proto_ref (frame
sequence and CLOSE rules) and utf8_ref (text messages)."""
import random
from collections import namedtuple

import numpy as np

import proto_ref as pr
import utf8_ref as ref

R = 6  # reads per connection
FORMS = ("separate", "unmask", "gather", "reframe", "reframe_masked")
IN_PLACE = ("separate", "unmask")
ERR_KINDS = {  # raw wire-level errors proto_ref's synthetic `err` cannot express -> the WSError they draw
    "unmasked": 7,   # a frame with payload and no mask (server mode)
    "len126": 6,     # a 126-class length below 126
    "len127": 6,     # a 127-class length with bit 63 set
    "ctl_long": 7,   # a control frame above 125 bytes
    "ctl_nofin": 7,  # a control frame without FIN
}
CUT_KINDS = ("hdr0", "ext2", "ext8", "key", "payload", "codepoint", "boundary", "empty", "noframe", "badlen_tail")
BIG = (65536, 65535)
MAX_FRAME = 10 * 1024 * 1024  # KMWS_MAX_FRAME_DATA_LENGTH

# frames: every frame on the wire as the references see it (a raw error is Fr(b0, b"", its WSError));
# layout[j] = (header offset, header bytes, payload bytes) of frames[j]; raw[j]: the raw error's kind or None
Conn = namedtuple("Conn", "frames wire reads layout raw")
Corpus = namedtuple("Corpus", "conns seed")
Got = namedtuple("Got", "b0 payload proto utf8 err")


# ------------------------------------------------------------------ corpus

def _xor(data, key):
    """proto_ref.mask_bytes for long payloads."""
    if not data:
        return b""
    a = np.frombuffer(data, dtype=np.uint8)
    return (a ^ np.resize(np.frombuffer(key, dtype=np.uint8), len(a))).tobytes()


def _raw_error(rng, kind):
    """-> (model frame, wire bytes, header bytes): one frame the server-mode parse refuses."""
    key = bytes(rng.randrange(256) for _ in range(4))
    if kind == "unmasked":
        b0 = rng.choice((0x81, 0x82, 0x80))
        return pr.Fr(b0, b"", 7), bytes([b0, 5]) + b"hello", 2
    if kind == "len126":
        b0, n = rng.choice((0x81, 0x82)), rng.choice((0, 5, 125))
        return pr.Fr(b0, b"", 6), bytes([b0, 0xFE, 0, n]) + key + bytes(n), 8
    if kind == "len127":
        b0 = rng.choice((0x81, 0x82))
        ext = rng.choice((bytes([0x80, 0, 0, 0, 0, 0, 0, 9]), bytes([0xFF] * 8), bytes([0x80, 0, 0, 0, 0, 1, 0, 0])))
        return pr.Fr(b0, b"", 6), bytes([b0, 0xFF]) + ext + key + b"123456789", 14
    if kind == "ctl_long":
        b0, n = rng.choice((0x89, 0x8A, 0x88)), rng.choice((126, 128, 300))
        return pr.Fr(b0, b"", 7), bytes([b0, 0xFE, n >> 8, n & 0xFF]) + key + bytes(n), 8
    assert kind == "ctl_nofin"
    b0 = rng.choice((0x09, 0x0A, 0x08))
    return pr.Fr(b0, b"", 7), bytes([b0, 0x83]) + key + b"abc", 6


_BAD_BYTES = (0xFF, 0xC0, 0x80, 0xED, 0xF5, 0xE0)


def _fill_text(rng, frames):
    """The fuzz's frames with real payloads of the same lengths: a text message
    is one well-formed string cut at the frame lengths (so code points straddle
    frames), now and then with one byte corrupted; everything else is noise."""
    out, mode, left = [], None, b""
    for f in frames:
        op, n = f.b0 & 15, len(f.payload)
        if op >= 8:
            out.append(f if op == 8 else f._replace(payload=bytes(rng.randrange(0x80, 0x100) for _ in range(n))))
            continue
        if op != 0:
            mode, left = ("text" if op == 1 and not f.b0 & 0x40 else "bin"), b""
        if mode == "text":
            if f.b0 & 0x80:  # the last fragment ends on a code point where there is room for it
                p = (left + ref.text(rng, n - len(left))) if len(left) <= n else left[:n]
                left = b""
            else:
                t = left + ref.text(rng, max(0, n - len(left)) + 3)
                p, left = t[:n], t[n:]
            if n and rng.random() < 0.06:
                p = bytearray(p)
                p[rng.randrange(n)] = rng.choice(_BAD_BYTES)
                p = bytes(p)
        else:
            p = bytes(rng.randrange(256) for _ in range(n))
        out.append(f._replace(payload=p))
        if f.b0 & 0x80:
            mode = None
    return out


def _encode(rng, frames, raws):
    wire, layout = bytearray(), []
    for f, raw in zip(frames, raws):
        if raw is not None:
            layout.append((len(wire), raw[1], len(raw[0]) - raw[1]))
            wire += raw[0]
            continue
        key = bytes(rng.randrange(256) for _ in range(4)) if rng.random() > 0.02 else b"\0\0\0\0"
        h = pr.wire_header(f.b0, len(f.payload), key)
        layout.append((len(wire), len(h), len(f.payload)))
        wire += pr.wire_of([f], lambda _: key) if len(f.payload) < 4096 else h + _xor(f.payload, key)
    return bytes(wire), layout


def _forced_cuts(rng, role, frames, layout, raw, n_ok):
    """Cut positions of one forced kind among the first n_ok frames (the ones
    in front of the connection's stop), or [] when the connection has no place for it."""
    idx = list(range(n_ok))
    rng.shuffle(idx)

    def first(pred):
        return next((j for j in idx if pred(j)), None)

    if role == "hdr0":
        j = first(lambda j: True)
        return [] if j is None else [layout[j][0] + 1]
    if role == "ext2":
        j = first(lambda j: layout[j][1] == 8)
        return [] if j is None else [layout[j][0] + 3]
    if role == "ext8":
        j = first(lambda j: layout[j][1] == 14)
        return [] if j is None else [layout[j][0] + 2 + rng.randint(1, 7)]
    if role == "key":
        j = first(lambda j: True)
        return [] if j is None else [layout[j][0] + layout[j][1] - rng.randint(1, 3)]
    if role == "payload":
        j = first(lambda j: layout[j][2] >= 2)
        return [] if j is None else [layout[j][0] + layout[j][1] + rng.randint(1, layout[j][2] - 1)]
    if role == "codepoint":
        for j in idx:
            p = frames[j].payload
            if frames[j].b0 & 0x4F == 0x01 and ref.valid(p):
                ks = [k for k in range(1, len(p)) if p[k] & 0xC0 == 0x80]
                if ks:
                    return [layout[j][0] + layout[j][1] + rng.choice(ks)]
        return []
    if role == "boundary":
        j = first(lambda j: j >= 1)
        return [] if j is None else [layout[j][0]]
    if role == "empty":
        j = first(lambda j: True)
        at = layout[j][0] + rng.randint(0, layout[j][1] + layout[j][2]) if j is not None else 0
        return [at, at]
    if role == "noframe":
        j = first(lambda j: layout[j][2] >= 3)
        if j is None:
            return []
        a = layout[j][0] + layout[j][1] + rng.randint(0, layout[j][2] - 3)
        return [a, a + rng.randint(1, 2)]
    if role == "raw" and raw in ("len126", "len127") and n_ok < len(layout):
        o = layout[n_ok][0]  # the refused header is the stop: cut inside it, or right behind its length bytes
        if raw == "len127":
            return [o + 2 + rng.randint(1, 7)]
        return [o + rng.choice((2, 3, 4))]
    return []


ROLES = ("hdr0", "ext2", "key", "raw", "payload", "codepoint", "boundary", "empty", "noframe", None, "raw", None,
         "payload", "codepoint", None, None)


def corpus(seed, n_conn):
    """n_conn connections -> Corpus.  A connection is a clean utf8_ref.random_stream
    prefix (half of them) and a proto_ref.fuzz_streams stream whose data frames
    carry real text; a synthetic `err` frame of the fuzz is replaced by one raw
    wire-level error (ERR_KINDS), which ends the wire.  Every 50th connection
    starts with a 65536- or 65535-byte message.  The masked server-mode wire is
    cut into R reads at random byte positions and at forced ones (CUT_KINDS) by
    the connection's role, index mod 16."""
    rng = random.Random(seed)
    streams = pr.fuzz_streams(seed, n_conn, rsv_allowed=pr.R1)
    kinds = list(ERR_KINDS)
    conns = []
    for i, s in enumerate(streams):
        role = ROLES[i % 16]
        frames = []
        if i % 50 == 9:
            n = BIG[(i // 50) % 2]
            frames.append(pr.Fr(0x81, ref.text(rng, n), 0) if (i // 100) % 2 else
                          pr.Fr(0x82, bytes(rng.randrange(256) for _ in range(n)), 0))
        if rng.random() < 0.5:
            frames += [pr.Fr(b0, p, 0) for b0, p in ref.random_stream(rng, rng.randint(1, 4), max_len=300)]
        body = s
        for j, f in enumerate(s):
            if f.err:
                body = s[:j]
                break
        frames += _fill_text(rng, body)
        raw_kind = None
        if role == "raw":  # every kind in turn, reached: nothing in front of it stops the connection
            frames = pr.deliverable(frames)
            if frames and frames[-1].b0 & 15 == 8:
                frames.pop()
            raw_kind = kinds[(i // 16) % len(kinds)] if i % 16 == 3 else ("len126", "len127")[(i // 16) % 2]
        elif len(body) < len(s):
            raw_kind = rng.choice(kinds)
        raws = [None] * len(frames)
        if raw_kind:
            model, data, hl = _raw_error(rng, raw_kind)
            frames.append(model)
            raws.append((data, hl))
        wire, layout = _encode(rng, frames, raws)
        n_ok = len(pr.deliverable(frames))
        cuts = _forced_cuts(rng, role, frames, layout, raw_kind, n_ok)
        if i % 50 == 9 and BIG[(i // 50) % 2] == 65536:
            cuts += _forced_cuts(rng, "ext8", frames, layout, raw_kind, n_ok)
        # half of the connections have every random cut in front of their stop, where the loops still read; the
        # others anywhere, so that they stop in an early round and leave the wire
        reach = layout[n_ok][0] + layout[n_ok][1] if n_ok < len(layout) and rng.random() < 0.5 else len(wire)
        while len(cuts) < R - 1:
            cuts.append(rng.randint(0, reach))
        cuts = [0] + sorted(cuts[:R - 1]) + [len(wire)]
        reads = [wire[a:b] for a, b in zip(cuts, cuts[1:])]
        conns.append(Conn(frames, wire, reads, layout, [None] * (len(frames) - 1) + [raw_kind] if raw_kind
                          else [None] * len(frames)))
    return Corpus(conns, seed)


def corpus_behind(seed, n_conn=24):
    """Connections that go on behind their stop: a clean prefix, then a valid
    CLOSE or a complete frame the parse refuses with a protocol error (which the
    walk steps over), then more frames.  For the device-only variant that keeps
    walking, as the descriptor-indexed parse allows."""
    rng = random.Random(seed)
    conns = []
    for i in range(n_conn):
        frames = [pr.Fr(b0, p, 0) for b0, p in ref.random_stream(rng, rng.randint(0, 3), max_len=200, p_corrupt=0)]
        raws = [None] * len(frames)
        raw_at = None
        if i % 2:
            frames.append(pr.close(rng.choice((1000, 1001, 3000)), rng.choice((b"", b"bye", "grüß".encode()))))
            raws.append(None)
        else:
            raw_kind = ("unmasked", "ctl_long", "ctl_nofin")[(i // 2) % 3]
            model, data, hl = _raw_error(rng, raw_kind)
            frames.append(model)
            raws.append((data, hl))
            raw_at = (len(frames) - 1, raw_kind)
        for _ in range(rng.randint(2, 6)):
            frames.append(rng.choice((pr.fr(pr.T, payload=b"late"), pr.fr(pr.PING, payload=b"?"), pr.close(1000),
                                      pr.fr(pr.C, 0, payload=b"xy"), pr.fr(pr.B, payload=bytes(130)), pr.fr(3))))
            raws.append(None)
        wire, layout = _encode(rng, frames, raws)
        cuts = [0] + sorted(rng.randint(0, len(wire)) for _ in range(R - 1)) + [len(wire)]
        raw = [None] * len(frames)
        if raw_at:
            raw[raw_at[0]] = raw_at[1]
        conns.append(Conn(frames, wire, [wire[a:b] for a, b in zip(cuts, cuts[1:])], layout, raw))
    return Corpus(conns, seed)


# ------------------------------------------------------------------ the host model of the loop

def host_parse(buf, h, end):
    """The server-mode header rules in the decoder's state order (HDR1, HDR2,
    extended length, key, payload; WSHandler.cpp:118-260) for the frame at
    buf[h:end] -> (WSError, b0, payload offset, length, key bytes).  1 = the
    bytes end before the rule that would decide."""
    if h >= end:
        return 1, 0, h, 0, b""
    b0 = buf[h]
    if not b0 & 0x80 and b0 & 0x08:
        return 7, b0, h, 0, b""
    if h + 2 > end:
        return 1, b0, h, 0, b""
    mask, plen = buf[h + 1] >> 7, buf[h + 1] & 0x7F
    if b0 & 0x08 and plen > 125:
        return 7, b0, h, 0, b""
    p = h + 2
    if plen == 126:
        if p + 2 > end:
            return 1, b0, h, 0, b""
        n = buf[p] << 8 | buf[p + 1]
        p += 2
        if n < 126:
            return 6, b0, h, 0, b""
    elif plen == 127:
        if p + 8 > end:
            return 1, b0, h, 0, b""
        x = 0
        for k in range(8):  # the reference's 32-bit shift, sign-extended (kmws_frame_parse.hpp ext_len127)
            v = (buf[p + k] << (((7 - k) * 8) & 31)) & 0xFFFFFFFF
            x |= v | (0xFFFFFFFF00000000 if v & 0x80000000 else 0)
        p += 8
        n = x & 0xFFFFFFFF
        if x >> 63 or n > MAX_FRAME:
            return 6, b0, h, 0, b""
    else:
        n = plen
    key = b""
    if mask:
        if p + 4 > end:
            return 1, b0, h, 0, b""
        key = bytes(buf[p:p + 4])
        p += 4
    elif n:
        return 7, b0, h, 0, b""
    if p + n > end:
        return 1, b0, h, 0, b""
    return 0, b0, p, n, key


def model_loop(corp, find_headers):
    """The device loop's bookkeeping on the host: per connection, per read, the
    frames completed [(b0, plain payload)], the failure code (0: none) and the
    tail held back.  find_headers: kmws.find_headers (the host walk)."""
    out = []
    for c in corp.conns:
        tail, rounds = b"", []
        for rd in c.reads:
            buf = tail + rd
            offs, used = find_headers(buf) if buf else ([], 0)
            if offs and offs[-1] == used:  # recorded, not consumed: the cut (or refused) frame is the tail
                offs = offs[:-1]
            got, fail, closed = [], 0, False
            for k, o in enumerate(offs):
                e, b0, p, n, key = host_parse(buf, o, offs[k + 1] if k + 1 < len(offs) else used)
                if e:
                    fail = e
                    break
                got.append((b0, _xor(bytes(buf[p:p + n]), key) if key else bytes(buf[p:p + n])))
                if b0 & 15 == 8:
                    closed = True
                    break
            tail = b"" if fail or closed else buf[used:]
            if tail:
                e = host_parse(tail, 0, len(tail))[0]
                assert e != 0, "the walk left a complete frame behind"
                if e != 1:
                    fail, tail = e, b""
            rounds.append((got, fail, tail))
            if fail or closed:
                break
        out.append(rounds)
    return out


# ------------------------------------------------------------------ the drop-in

def handler_loop(corp):
    """Per connection a kmws.WSHandler(SERVER) with both checks on, fed the
    connection's reads -> per connection, per read, (return code, [Got]); a
    connection is dropped after an error return or a delivered CLOSE."""
    from kuma_amd import kmws
    out = []
    for c in corp.conns:
        h = kmws.WSHandler(kmws.SERVER)
        h.setUtf8Check(True)
        h.set_proto_check(True, pr.R1)
        got = []

        def cb(hd, p, h=h, got=got):
            b0 = hd.fin << 7 | hd.rsv1 << 6 | hd.rsv2 << 5 | hd.rsv3 << 4 | hd.opcode
            got.append(Got(b0, p, h.last_frame_proto(), hd.utf8, 0))

        h.setFrameCallback(cb)
        rounds = []
        for rd in c.reads:
            del got[:]
            rc = h.handleData(rd)
            rounds.append((rc, list(got)))
            if rc not in (0, 1) or any(g.b0 & 15 == 8 for g in got):
                break
        out.append(rounds)
    return out


# ------------------------------------------------------------------ the device loop

class DeviceRun:
    """What device_loop saw: per connection, per round, rounds[c][r] = [frames
    [Got], failure code, tail bytes, per frame (relayed bytes, outgoing key) or
    None, bytes fed so far]; the two final carries."""

    def __init__(self, n):
        self.rounds = [[] for _ in range(n)]
        self.ucarry = np.zeros((n, 8), dtype=np.uint8)
        self.pcarry = np.zeros((n, 8), dtype=np.uint8)
        self.n_rounds = 0
        self.n_classified = 0
        self.flat_fail = set()  # connections that failed on a frame of the flat list (not on their tail)
        self.max_live = self.max_frames = 0


def device_loop(corp, form, cap, proto_first, stop=True):
    """INTEGRATION.md section 2's loop over the entries of kmws_gpu.h.  Each
    round: every live connection's held-back tail plus its new read, back to back
    in one wire (16 bytes of slack behind it) -> kmws_find_headers_streams(cap)
    -> the flat hdr_off / stream_first, built on the host -> one payload pass
    (`form`) with the connections' UTF-8 carries -> kmws_proto_check on that
    call's out_desc / out_flags / out_err with their proto carries (before the
    pass when proto_first; payload_masked says what the wire holds then) -> the
    tails copied back from the device wire.

    Compaction: a stream's last recorded frame is left out iff its offset is
    lo + consumed -- the walk records a frame it cannot step over (cut, or an
    invalid length) without consuming it.  That frame is the connection's tail,
    and the tail is never put into the flat list: the parse bounds a frame's
    payload by the next header offset but its header bytes only by wire_len, so
    a cut header in front of another connection's bytes would be completed with
    them (tail `81`, neighbour `FE 00 05`: a bad length).  Instead one
    kmws_unpack_headers call per non-empty tail -- n = 1, wire_len = the
    stream's end, so no neighbouring byte can be read -- tells "cut, wait"
    (NEED_MORE_DATA, 1) from "refused, fail now" (anything else), which the
    walk's outputs alone do not.

    A frame of the flat list with out_err != 0 fails its connection at that
    frame; a CLOSE ends it (stop=False: keep walking behind both, as the
    descriptor-indexed parse allows).  Workspaces and outputs are allocated once
    and reused, so every round runs over the previous round's contents; every
    status word is asserted.  After the last read, empty rounds follow until no
    tail holds a complete frame (a small cap lags behind the reads)."""
    import torch as T
    from kuma_amd import kmws
    conns = corp.conns
    nc = len(conns)
    total_bytes = sum(len(c.wire) for c in conns)
    N = sum(len(c.frames) for c in conns) + 1
    cap_w = (total_bytes + 16 + 15) // 16 * 16
    cap_d = (total_bytes + 14 * N + 32 + 15) // 16 * 16
    dev = "cuda"
    wire_d = T.full((cap_w,), 0xA5, dtype=T.uint8, device=dev)
    hdr_d = T.full((nc, cap), -1, dtype=T.int64, device=dev)
    desc_d = T.full((N, 2), -1, dtype=T.int64, device=dev)
    flags_d = T.full((N,), -1, dtype=T.int16, device=dev)
    err_d = T.full((N,), 0xEE, dtype=T.uint8, device=dev)
    utf8_d = T.full((N,), 0xEE, dtype=T.uint8, device=dev)
    proto_d = T.full((N,), 0xEE, dtype=T.uint8, device=dev)
    cls_desc = T.full((nc, 2), -1, dtype=T.int64, device=dev)
    cls_err = T.full((nc,), 0xEE, dtype=T.uint8, device=dev)
    dst_d = off_d = okeys_d = okeys = None
    if form not in IN_PLACE:
        dst_d = T.full((cap_d,), 0x5A, dtype=T.uint8, device=dev)
        off_d = T.full((N + 1,), -1, dtype=T.int64, device=dev)
    if form == "reframe_masked":
        okeys = np.random.default_rng(corp.seed).integers(0, 2**32, size=N, dtype=np.uint64).astype(np.uint32)
        okeys_d = T.from_numpy(okeys.view(np.int32).copy()).to(dev)
    unpack_bytes = kmws.lib().kmws_unpack_workspace_size()
    ws_unpack, ws_cls = kmws.Workspace(unpack_bytes), kmws.Workspace(unpack_bytes)
    ws_proto = kmws.Workspace(max(kmws.proto_workspace_size(N, nc), kmws.proto_workspace_size(1, 1)))
    if form == "separate":
        ws_utf8 = kmws.Workspace(kmws.utf8_workspace_size(cap_w, N, nc))
        ws_pass = kmws.Workspace(kmws.unmask_workspace_size(cap_w))
    elif form == "unmask":
        ws_pass = kmws.Workspace(kmws.unmask_utf8_workspace_size(cap_w, N, nc))
    elif form == "gather":
        ws_pass = kmws.Workspace(kmws.gather_utf8_workspace_size(N, cap_d, nc))
    else:
        ws_pass = kmws.Workspace(kmws.reframe_utf8_workspace_size(N, cap_d, nc))

    run = DeviceRun(nc)
    live, tails, fed = list(range(nc)), [b""] * nc, [0] * nc
    rnd = 0
    while rnd < R or any(tails[c] for c in live):
        assert rnd < R + N, "the tails do not drain"
        pieces = [tails[c] + (conns[c].reads[rnd] if rnd < R else b"") for c in live]
        progress = rnd < R
        for c, p in zip(live, pieces):
            fed[c] += len(p) - len(tails[c])
        ns = len(live)
        soff = np.zeros(ns + 1, dtype=np.int64)
        soff[1:] = np.cumsum([len(p) for p in pieces])
        total = int(soff[-1])
        flat, first, cut, cons = [], [0], [False] * ns, np.zeros(ns, dtype=np.int64)
        if total:
            wire_d[:total].copy_(T.from_numpy(np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()))
            _, n_out, consumed = kmws.find_headers_streams(wire_d, T.from_numpy(soff).to(dev), cap, wire_len=total,
                                                           hdr=hdr_d[:ns])
            n_out, cons, H = n_out.cpu().numpy(), consumed.cpu().numpy(), hdr_d[:ns].cpu().numpy()
            for s in range(ns):
                k = int(n_out[s])
                assert k <= cap and 0 <= cons[s] <= soff[s + 1] - soff[s]
                if k and H[s, k - 1] == soff[s] + cons[s]:
                    k, cut[s] = k - 1, True
                flat.extend(int(x) for x in H[s, :k])
                first.append(len(flat))
        else:
            first += [0] * ns
        n = len(flat)
        run.max_live, run.max_frames = max(run.max_live, ns), max(run.max_frames, n)
        uc_in, pc_in = run.ucarry[live], run.pcarry[live]
        uc_out, pc_out = uc_in, pc_in  # no frame in the whole round: nothing is called, the carries stay
        if n:
            progress = True
            hoff_d = T.tensor(flat, dtype=T.int64, device=dev)
            first_d = T.tensor(first, dtype=T.int32, device=dev)
            desc, flags, err, utf8, proto = desc_d[:n], flags_d[:n], err_d[:n], utf8_d[:n], proto_d[:n]
            ci_u, ci_p = T.from_numpy(uc_in.copy()).to(dev), T.from_numpy(pc_in.copy()).to(dev)
            co_u = T.full((ns, 8), 0xEE, dtype=T.uint8, device=dev)
            co_p = T.full((ns, 8), 0xEE, dtype=T.uint8, device=dev)
            streams = dict(stream_first=first_d, carry_in=ci_u, carry_out=co_u)

            def parse_status(ws, what):
                want = 2 if bool(err.any()) else 0
                got = ws.status()
                assert got == want, f"round {rnd}: {what} left status {got}, want {want}"

            def check_proto(masked):
                kmws.proto_check(wire_d, desc, flags, proto, ws_proto, err=err, span=total, masked=masked,
                                 rsv_allowed=pr.R1, stream_first=first_d, carry_in=ci_p, carry_out=co_p)
                assert ws_proto.status() == 0, f"round {rnd}: kmws_proto_check status"

            parsed = None
            if form == "separate" or proto_first:
                kmws.unpack_headers(wire_d, hoff_d, kmws.SERVER, desc, flags, err, ws_unpack, wire_len=total)
                parse_status(ws_unpack, "kmws_unpack_headers")
                parsed = (desc.clone(), flags.clone(), err.clone())
            if proto_first:
                check_proto(True)
            if form == "separate":
                kmws.utf8_validate(wire_d, desc, flags, utf8, ws_utf8, span=total, masked=True, **streams)
                assert ws_utf8.status() == 0, f"round {rnd}: kmws_utf8_validate status"
                kmws.unmask_batch(wire_d, desc, ws_pass, span=total)
                assert ws_pass.status() == 0, f"round {rnd}: kmws_unmask_batch status"
            elif form == "unmask":
                kmws.unpack_unmask_utf8(wire_d, hoff_d, kmws.SERVER, desc, flags, err, utf8, ws_pass, wire_len=total,
                                        **streams)
                parse_status(ws_pass, "kmws_unpack_unmask_utf8")
            elif form == "gather":
                kmws.unpack_gather_utf8(wire_d, hoff_d, kmws.SERVER, desc, flags, err, dst_d, off_d[:n + 1], utf8,
                                        ws_pass, wire_len=total, **streams)
                parse_status(ws_pass, "kmws_unpack_gather_utf8")
            else:
                kmws.unpack_reframe_utf8(wire_d, hoff_d, kmws.SERVER, desc, flags, err, 0x0007,
                                         form == "reframe_masked", okeys_d[:n] if okeys_d is not None else None,
                                         dst_d, off_d[:n + 1], utf8, ws_pass, wire_len=total, **streams)
                parse_status(ws_pass, "kmws_unpack_reframe_utf8")
            if parsed is not None:
                assert T.equal(desc, parsed[0]) and T.equal(flags, parsed[1]) and T.equal(err, parsed[2]), \
                    f"round {rnd}: the fused parse differs from kmws_unpack_headers"
            if not proto_first:
                check_proto(form not in IN_PLACE)
            uc_out, pc_out = co_u.cpu().numpy(), co_p.cpu().numpy()
            D = desc.cpu().numpy()
            d_off, d_len, d_key = D[:, 0], D[:, 1] & 0xFFFFFFFF, (D[:, 1] >> 32) & 0xFFFFFFFF
            F, E = flags.cpu().numpy().view(np.uint16), err.cpu().numpy()
            U, P = utf8.cpu().numpy(), proto.cpu().numpy()
            if dst_d is not None:
                O = off_d[:n + 1].cpu().numpy()
                dst = dst_d[:int(O[n])].cpu().numpy()
        after = wire_d[:total].cpu().numpy() if total else np.zeros(0, dtype=np.uint8)

        ended, classify = set(), []
        for s, c in enumerate(live):
            got, relay, fail = [], [], 0
            for k in range(first[s], first[s + 1]):
                b0 = int(F[k]) & 0xFF
                if E[k]:
                    if stop:
                        fail = int(E[k])
                        break
                    got.append(Got(b0, b"", int(P[k]), int(U[k]), int(E[k])))
                    continue
                o, ln = int(d_off[k]), int(d_len[k])
                assert soff[s] <= o and o + ln <= soff[s] + cons[s], "a descriptor leaves its stream"
                if form in IN_PLACE:
                    payload = after[o:o + ln].tobytes()
                elif form == "gather":
                    assert int(O[k + 1] - O[k]) == ln
                    payload = dst[int(O[k]):int(O[k + 1])].tobytes()
                else:  # the wire is untouched: unmask it here; the relayed bytes are compared by the caller
                    payload = _xor(after[o:o + ln].tobytes(), int(d_key[k]).to_bytes(4, "little"))
                    relay.append((dst[int(O[k]):int(O[k + 1])].tobytes(),
                                  int(okeys[k]).to_bytes(4, "little") if okeys is not None else None))
                got.append(Got(b0, payload, int(P[k]), int(U[k]), 0))
                if b0 & 15 == 8 and stop:
                    ended.add(c)
                    break
            if fail:
                ended.add(c)
            tail = b"" if c in ended else after[int(soff[s] + cons[s]):int(soff[s + 1])].tobytes()
            if fail:
                run.flat_fail.add(c)
            run.rounds[c].append([got, fail, tail, relay if form not in IN_PLACE else None, fed[c]])
            if tail and cut[s]:
                classify.append((s, c))
            if first[s + 1] > first[s]:
                run.ucarry[c], run.pcarry[c] = uc_out[s], pc_out[s]
            else:  # an empty stream: the entries must have passed its carries through
                assert bytes(uc_out[s]) == bytes(run.ucarry[c]) and bytes(pc_out[s]) == bytes(run.pcarry[c]), \
                    f"round {rnd}: an empty stream's carry changed"
            tails[c] = tail
        if classify:
            t_off = T.tensor([int(soff[s] + cons[s]) for s, _ in classify], dtype=T.int64, device=dev)
            sts = []
            for j, (s, c) in enumerate(classify):
                kmws.unpack_headers(wire_d, t_off[j:j + 1], kmws.SERVER, cls_desc[j:j + 1], None, cls_err[j:j + 1],
                                    ws_cls, wire_len=int(soff[s + 1]))
                sts.append(ws_cls.status())
            ce = cls_err[:len(classify)].cpu().numpy()
            run.n_classified += len(classify)
            for j, (s, c) in enumerate(classify):
                e = int(ce[j])
                assert e != 0, "the walk left a complete frame unconsumed"
                assert sts[j] == 2, f"round {rnd}: the tail's parse left status {sts[j]}"
                if e != 1:
                    run.rounds[c][-1][1], run.rounds[c][-1][2] = e, b""
                    tails[c] = b""
                    ended.add(c)
        live = [c for c in live if c not in ended]
        rnd += 1
        if not progress:
            break
    run.n_rounds = rnd
    return run
