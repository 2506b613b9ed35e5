"""Cases and runners shared by the tests that pin the oracle and the device
paths to the built reference (oracle/ref_build.py), and by the recorder of
tests/golden/reference_recorded.json.  Plain Python + numpy: no torch, no GPU.

A *backend* is anything with the surface of oracle.oracle: the module itself
(the restatement) or oracle.reference("O3" / "O0") (kuma's compiled
WSHandler.cpp).  A decode *case* is a dict in the schema of
tests/golden/reference_vectors.json, extended by

    destroy_on     the frame callback destroys the handler at this frame index
    then[i].op     "reset" or "set_mode" (with "mode") instead of a feed
    then[i].chunk  feed that step's bytes in pieces of this size (0: whole)

`run_case` gives every observable of a case on one backend: each feed's return
code, the frame count after it, the caller's buffer after it (in-place unmask)
and all eleven fields of every frame.  A handler its callback destroyed is not
fed again: the run stops at the first DESTROYED, on every backend alike (the
reference object is gone; there is no behaviour to compare).
"""
import hashlib
import random

from oracle import oracle as orc

CLIENT, SERVER = orc.CLIENT, orc.SERVER
MODES = {"CLIENT": CLIENT, "SERVER": SERVER}
MAX_LEN = 10 * 1024 * 1024
DESTROYED = 9

HELLO = "48656c6c6f"
KEY = "37fa213d"
MASKED_HELLO = KEY + "7f9f4d5158"


def gen(name, n):
    if name == "zeros":
        return bytes(n)
    if name == "iota":
        return bytes(range(256)) * (n // 256) + bytes(range(n % 256))
    raise ValueError(name)


def step_input(c):
    data = bytes.fromhex(c.get("input_hex", ""))
    if "tail_gen" in c:
        data += gen(c["tail_gen"], c["tail_len"])
    return data


# ------------------------------ runner ------------------------------
class Run:
    """rets / counts / buffers: one entry per feed, over the whole case; frames:
    Frame.key() of every callback; groups: the feeds of the case's own input
    first, then of each `then` step (for the recorded fixture)."""

    def __init__(self):
        self.rets, self.counts, self.buffers, self.frames, self.groups = [], [], [], [], []

    def observables(self):
        return self.rets, self.counts, self.buffers, self.frames


def _feed_pieces(d, run, data, chunk):
    """False once the handler is destroyed."""
    pieces = [data] if chunk <= 0 else [data[i:i + chunk] for i in range(0, len(data), chunk)]
    group = []
    run.groups.append(group)
    for p in pieces:
        buf = bytearray(p)
        ret = d.feed(buf)
        run.rets.append(ret)
        group.append(ret)
        run.counts.append(len(d.frames))
        run.buffers.append(bytes(buf))
        if ret == DESTROYED:
            return False
    return True


def run_case(backend, c):
    d = backend.Decoder(MODES[c["mode"]])
    d.destroy_on = c.get("destroy_on")
    run = Run()
    alive = _feed_pieces(d, run, step_input(c), c["chunk"])
    for st in c.get("then", []):
        if not alive:
            break
        if st.get("op") == "reset":
            d.reset()
        elif st.get("op") == "set_mode":
            d.set_mode(MODES[st["mode"]])
        else:
            alive = _feed_pieces(d, run, step_input(st), st.get("chunk", 0))
    run.frames = [f.key() for f in d.frames]
    return run


def run_stream(backend, mode, stream, cut, destroy_on=None):
    """One stream cut into `cut`-byte feeds (0: whole)."""
    d = backend.Decoder(mode)
    d.destroy_on = destroy_on
    run = Run()
    _feed_pieces(d, run, stream, cut)
    run.frames = [f.key() for f in d.frames]
    return run


# ------------------------------ frames ------------------------------
def wire_frame(backend, b0, mask, length, key=b"\0\0\0\0", payload=None):
    """encodeFrameHeader + masked payload through `backend`."""
    h = orc.Hdr(fin=b0 >> 7, rsv1=(b0 >> 6) & 1, rsv2=(b0 >> 5) & 1, rsv3=(b0 >> 4) & 1,
                opcode=b0 & 15, mask=mask, maskey=key, length=length)
    payload = bytes(length) if payload is None else payload
    return backend.encode_header(h) + (backend.mask_bytes(key, payload) if mask else payload)


def hdr_len(length, mask):
    return (2 if length <= 125 else 4 if length <= 0xFFFF else 10) + (4 if mask else 0)


# ------------------------------ streaming-state cases ------------------------------
def _case(name, mode, input_hex, chunk=0, then=None, destroy_on=None, tail_gen=None, tail_len=0):
    c = dict(name=name, source="recorded", mode=mode, input_hex=input_hex, chunk=chunk)
    if tail_gen:
        c["tail_gen"], c["tail_len"] = tail_gen, tail_len
    if destroy_on is not None:
        c["destroy_on"] = destroy_on
    if then:
        c["then"] = then
    return c


def _feed(input_hex, chunk=0):
    st = dict(input_hex=input_hex)
    if chunk:
        st["chunk"] = chunk
    return st


RESET = dict(op="reset")


def streaming_cases():
    """The streaming-state cases (inputs only; run_case or the recorder adds the
    expectations).  Frames are written out in hex by hand, not encoded by any
    backend, so the inputs do not depend on what is under test."""
    S, Cm = "SERVER", "CLIENT"
    good_s = "8185" + MASKED_HELLO          # masked text "Hello"
    good_c = "8105" + HELLO
    cases = [
        _case("close_then_trailing_same_feed", Cm, "880203e8" + good_c, then=[_feed(good_c), _feed("")]),
        _case("close_then_trailing_bytewise", S, "8882" + KEY + "3412" + good_s, chunk=1,
              then=[_feed(good_s, 1)]),
        _case("close_empty_then_reset", Cm, "8800", then=[_feed(good_c), RESET, _feed(good_c)]),
    ]
    errors = [
        ("control_not_fin", Cm, "0900"),
        ("control_plen_126", Cm, "897e007e"),
        ("control_plen_127", S, "8aff0000000000000001"),
        ("len16_below_126", Cm, "827e007d"),
        ("len64_bit63", Cm, "827f8000000000000000"),
        ("len64_sign_from_byte4", Cm, "827f0000000080000000"),
        ("len64_cap_plus_1", Cm, "827f0000000000a00001"),
        ("masked_in_client", Cm, good_s),
        ("unmasked_in_server", S, good_c),
    ]
    for name, mode, bad in errors:
        good = good_s if mode == S else good_c
        for chunk in (0, 1):
            cases.append(_case(f"error_{name}_more_reset_valid_chunk{chunk}", mode, bad, chunk=chunk,
                               then=[_feed(good), _feed("00"), RESET, _feed(good, chunk), _feed(good)]))
    # set_mode between frames and mid-header (after byte 1, inside the extended
    # length, inside the key: the mask rule is read when the key state is reached)
    cases += [
        _case("set_mode_between_frames", S, good_s,
              then=[dict(op="set_mode", mode=Cm), _feed(good_c), _feed(good_s)]),
        _case("set_mode_between_frames_to_server", Cm, good_c,
              then=[dict(op="set_mode", mode=S), _feed(good_s), _feed(good_c)]),
        _case("set_mode_after_byte1", S, "81", then=[dict(op="set_mode", mode=Cm), _feed("05" + HELLO)]),
        _case("set_mode_after_byte2_masked", Cm, "8185",
              then=[dict(op="set_mode", mode=S), _feed(MASKED_HELLO)]),
        _case("set_mode_inside_length", S, "81fe00", then=[dict(op="set_mode", mode=Cm), _feed("7e" + KEY)]),
        _case("set_mode_inside_key", S, "8185" + KEY[:4],
              then=[dict(op="set_mode", mode=Cm), _feed(KEY[4:] + "7f9f4d5158"), _feed(good_c)]),
        _case("set_mode_inside_payload", S, "8185" + KEY + "7f9f",
              then=[dict(op="set_mode", mode=Cm), _feed("4d5158"), _feed(good_c)]),
    ]
    # a header cut at each of its byte positions: 14 bytes (masked, 127-class, a
    # non-minimal length 3) and 8 bytes (masked, 126-class)
    h14 = "82ff0000000000000003" + KEY + "aabbcc"
    h8 = "81fe007e" + KEY
    for k in range(1, 15):
        cases.append(_case(f"header14_cut_at_{k:02d}", S, h14[:2 * k], then=[_feed(h14[2 * k:]), _feed(good_s)]))
    for k in range(1, 9):
        c = _case(f"header8_cut_at_{k}", S, h8[:2 * k], then=[dict(input_hex=h8[2 * k:], tail_gen="iota",
                                                                   tail_len=126)])
        cases.append(c)
    # reset in the middle of a header and of a payload
    cases += [
        _case("reset_inside_length", S, "82ff000000", then=[RESET, _feed(good_s)]),
        _case("reset_inside_payload", S, "8185" + KEY + "7f9f", then=[RESET, _feed(good_s)]),
    ]
    # a payload in three feeds (the reassembly buffer), masked and unmasked,
    # followed in the last feed by another frame
    cases += [
        _case("payload_three_feeds_masked", S, "8185" + KEY + "7f", then=[_feed("9f4d"), _feed("5158" + good_s)]),
        _case("payload_three_feeds_unmasked", Cm, "810548", then=[_feed("656c"), _feed("6c6f" + good_c)]),
        _case("payload_300_chunk_7", S, "82fe012c" + KEY, chunk=7, tail_gen="iota", tail_len=300),
        _case("payload_70000_chunk_4096", S, "82ff0000000000011170" + KEY, chunk=4096, tail_gen="iota",
              tail_len=70000),
    ]
    # the cap and one above it
    cases += [
        _case("cap_10MiB_unmasked", Cm, "827f0000000000a00000", tail_gen="iota", tail_len=MAX_LEN),
        _case("cap_10MiB_masked_two_feeds", S, "82ff0000000000a00000" + KEY, chunk=MAX_LEN // 2 + 7,
              tail_gen="iota", tail_len=MAX_LEN),
        _case("cap_plus_1_masked", S, "82ff0000000000a00001" + KEY, tail_gen="zeros", tail_len=64,
              then=[_feed(good_s), RESET, _feed(good_s)]),
    ]
    # the callback destroys the handler
    three = good_s + "8285" + KEY + "0011223344" + "8985" + MASKED_HELLO
    cases += [
        _case("destroy_at_frame_0", S, three, destroy_on=0, then=[_feed(good_s)]),
        _case("destroy_at_middle_frame", S, three, destroy_on=1, then=[_feed(good_s)]),
        _case("destroy_at_middle_frame_bytewise", S, three, chunk=1, destroy_on=1),
        _case("destroy_at_close", S, good_s + "8882" + KEY + "3412" + good_s, destroy_on=1, then=[_feed(good_s)]),
        _case("destroy_at_reassembled_frame", S, "8185" + KEY + "7f", destroy_on=0,
              then=[_feed("9f4d5158" + good_s)]),
    ]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


# ------------------------------ encode table ------------------------------
ENCODE_LENGTHS = (0, 1, 125, 126, 127, 65535, 65536, 65537, 1 << 24, MAX_LEN, MAX_LEN + 1, 1 << 31, (1 << 32) - 1)
ENCODE_KEY = bytes.fromhex("deadbe00")  # a zero byte in the key


def encode_table_full():
    """Every first byte x mask x ENCODE_LENGTHS: (b0, mask, key, length)."""
    return [(b0, mask, ENCODE_KEY if mask else b"\0\0\0\0", L)
            for b0 in range(256) for mask in (0, 1) for L in ENCODE_LENGTHS]


FIXTURE_B0 = tuple((fl << 4) | op for fl in range(16) for op in (0, 2, 9, 15))  # the 64 of the fixture


def encode_table_fixture():
    """The recorded subset: four first bytes x mask x every length, and the 64
    flag/opcode combinations x mask at one length of the 7-bit and of the
    127 class."""
    rows = [(b0, mask, L) for b0 in (0x82, 0x01, 0xF9, 0x0F) for mask in (0, 1) for L in ENCODE_LENGTHS]
    rows += [(b0, mask, L) for b0 in FIXTURE_B0 for mask in (0, 1) for L in (5, 65536)]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append((r[0], r[1], ENCODE_KEY if r[1] else b"\0\0\0\0", r[2]))
    return out


def encode_case(b0, mask, key, length):
    return dict(name=f"b0_{b0:02x}_mask{mask}_len{length}", source="recorded", fin=b0 >> 7, rsv1=(b0 >> 6) & 1,
                rsv2=(b0 >> 5) & 1, rsv3=(b0 >> 4) & 1, opcode=b0 & 15, mask=mask, maskey=key.hex(), length=length)


def encode_run(backend, c):
    h = orc.Hdr(fin=c["fin"], rsv1=c["rsv1"], rsv2=c["rsv2"], rsv3=c["rsv3"], opcode=c["opcode"],
                mask=c["mask"], maskey=bytes.fromhex(c["maskey"]), length=c["length"])
    return backend.encode_header(h).hex()


# ------------------------------ mask table ------------------------------
MASK_KEYS = (bytes.fromhex("37fa213d"), bytes.fromhex("a100c3d4"), bytes(4))
MASK_MAX_LEN = 67
_FEW_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 67)


def mask_data(n, salt=0):
    return bytes((37 * i + 11 * salt + 5) & 0xFF for i in range(n))


def mask_table_full():
    """(key, length, phase) for every length 0..67 x phase 0..7 x the three keys."""
    return [(k, n, ph) for k in MASK_KEYS for n in range(MASK_MAX_LEN + 1) for ph in range(8)]


def mask_table_fixture():
    """The recorded subset (the file has a size limit): the first key at every
    length x phase 0..1 and at the edge lengths x phase 2..7; the other two keys
    at the edge lengths x phase 0, 1, 3."""
    k0 = MASK_KEYS[0]
    rows = [(k0, n, ph) for n in range(MASK_MAX_LEN + 1) for ph in range(2)]
    rows += [(k0, n, ph) for n in _FEW_LENS for ph in range(2, 8)]
    rows += [(k, n, ph) for k in MASK_KEYS[1:] for n in _FEW_LENS for ph in (0, 1, 3)]
    return rows


def chain_cases():
    """Chains of 1..5 segments with empty segments inside: (key, [segments])."""
    rng = random.Random(0x4348414E)
    sizes = (0, 0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 33)
    out = []
    for key in MASK_KEYS:
        for nseg in range(1, 6):
            for rep in range(6):
                segs = [mask_data(rng.choice(sizes), rng.randrange(256)) for _ in range(nseg)]
                if rep == 0:
                    segs[0] = b""                      # an empty head
                if rep == 1:
                    segs[-1] = b""                     # an empty tail
                if rep == 2 and nseg >= 3:
                    segs[1] = b""                      # an empty one inside
                    segs[0] = segs[0] or b"\x01\x02\x03"
                if rep == 3:
                    segs = [b""] * nseg                # nothing but empty ones
                out.append((key, segs))
    return out


def mask_case(key, n, phase):
    """The fixture's form: a chain whose first segment holds `phase` bytes."""
    segs = ([mask_data(phase, 99)] if phase else []) + [mask_data(n, n)]
    return dict(name=f"key_{key.hex()}_len{n}_phase{phase}", source="recorded", key=key.hex(),
                segments_hex=[s.hex() for s in segs])


def mask_run(backend, c):
    return [s.hex() for s in backend.mask_chain(bytes.fromhex(c["key"]), [bytes.fromhex(s) for s in c["segments_hex"]])]


# ------------------------------ recording ------------------------------
def frame_record(key):
    """A Frame.key() as the fixture stores it: payloads above 256 bytes by
    generator name where one matches, and always by SHA-256."""
    fin, rsv1, rsv2, rsv3, opcode, mask, plen, xpl64, maskey, length, payload = key
    f = dict(fin=fin, rsv1=rsv1, rsv2=rsv2, rsv3=rsv3, opcode=opcode, mask=mask, plen=plen, xpl64=xpl64,
             maskey=maskey.hex(), length=length)
    if len(payload) <= 256:
        f["payload_hex"] = payload.hex()
    else:
        for g in ("zeros", "iota"):
            if payload == gen(g, len(payload)):
                f["payload_gen"] = g
        f["payload_sha256"] = hashlib.sha256(payload).hexdigest()
    return f


def record_decode(backend, c):
    """`c` with the expectations `backend` gives: expect_rets / expect_frames
    for the case's own input (frames: all of the case, `then` steps included),
    expect_rets per `then` feed."""
    run = run_case(backend, c)
    out = {k: v for k, v in c.items() if not k.startswith("expect_")}
    groups = list(run.groups)
    out["expect_rets"] = groups.pop(0)
    out["expect_frames"] = [frame_record(k) for k in run.frames]
    then = []
    for st in c.get("then", []):
        st = {k: v for k, v in st.items() if k != "expect_rets"}
        if "op" not in st:
            st["expect_rets"] = groups.pop(0) if groups else []   # []: the handler was destroyed before
        then.append(st)
    if then:
        out["then"] = then
    return out


def check_decode(backend, c):
    """Assert that `backend` gives what the recorded case `c` holds."""
    want = c
    got = record_decode(backend, c)
    assert got["expect_rets"] == want["expect_rets"], (c["name"], got["expect_rets"], want["expect_rets"])
    assert len(got["expect_frames"]) == len(want["expect_frames"]), c["name"]
    for g, w in zip(got["expect_frames"], want["expect_frames"]):
        for k, v in w.items():
            if k == "payload_gen":
                assert g.get("payload_gen") == v or g["payload_sha256"] == hashlib.sha256(
                    gen(v, w["length"])).hexdigest(), (c["name"], k)
            else:
                assert g.get(k) == v, (c["name"], k, g.get(k), v)
    for g, w in zip(got.get("then", []), want.get("then", [])):
        assert g.get("expect_rets") == w.get("expect_rets"), (c["name"], g, w)


# ------------------------------ fuzz ------------------------------
FUZZ_SEED = 0x46555A5A
FUZZ_STREAMS = 2000
FUZZ_LENGTHS = (0, 1, 5, 125, 126, 127, 300, 65535, 65536, 70000)
FUZZ_LENGTH_WEIGHTS = (4, 4, 6, 4, 4, 4, 4, 1, 1, 1)
FUZZ_CUTS = (1, 2, 3, 7, 13, 4096, 0)
FUZZ_OPCODES = (0, 1, 2, 1, 2, 3, 7, 8, 9, 10, 11, 15)


def fuzz_streams(seed=FUZZ_SEED, n=FUZZ_STREAMS):
    """[(mode, stream, cut, destroy_on)].  The mix: streams of 1-6 items; an item
    is a valid frame (a length of FUZZ_LENGTHS, an opcode of FUZZ_OPCODES, random
    flag bits; masked as the mode wants it 9 times in 10), of which 15 % get one
    extended-length byte corrupted and 10 % a truncated payload, or (25 %) a run
    of 1-40 random bytes.  One run in ten destroys the handler at frame 0, 1 or
    2.  The cut is drawn from FUZZ_CUTS; a stream above 16 KiB does not take the
    cuts below 13, which would only repeat the same path tens of thousands of
    times.  Frames are built in plain Python (no backend)."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        mode = rng.choice((CLIENT, SERVER))
        parts = []
        for _ in range(rng.randint(1, 6)):
            if rng.random() < 0.25:
                parts.append(bytes(rng.randrange(256) for _ in range(rng.randint(1, 40))))
                continue
            L = rng.choices(FUZZ_LENGTHS, FUZZ_LENGTH_WEIGHTS)[0]
            op = rng.choice(FUZZ_OPCODES)
            fin = 1 if op >= 8 and rng.random() < 0.9 else rng.randrange(2)
            b0 = (fin << 7) | (rng.randrange(8) << 4 if rng.random() < 0.2 else 0) | op
            mask = (mode == SERVER) if rng.random() < 0.9 else (mode != SERVER)
            key = bytes(rng.randrange(256) for _ in range(4))
            m = 0x80 if mask else 0
            if L <= 125:
                hdr = bytes([b0, m | L])
            elif L <= 0xFFFF:
                hdr = bytes([b0, m | 126]) + L.to_bytes(2, "big")
            else:
                hdr = bytes([b0, m | 127]) + L.to_bytes(8, "big")
            if L > 125 and rng.random() < 0.15:
                k = rng.randrange(2, len(hdr))
                hdr = hdr[:k] + bytes([rng.randrange(256)]) + hdr[k + 1:]
            payload = rng.randbytes(L)
            if L and rng.random() < 0.10:
                payload = payload[:rng.randrange(L)]
            parts.append(hdr + (key if mask else b"") + payload)
        stream = b"".join(parts)
        cuts = FUZZ_CUTS if len(stream) <= 16384 else (13, 4096, 0)
        destroy_on = rng.randrange(3) if rng.random() < 0.1 else None
        out.append((mode, stream, rng.choice(cuts), destroy_on))
    return out
