"""The UTF-8 check of text frames on the resident worker (the launch-free
path): with kmws_decoder_set_utf8_check on, kmws_decoder_feed,
kmws_decoder_feed_deferred and kmws_rx_batch_* post checked jobs on the grid,
whose validating instantiation unmasks and validates in one pass
(kuma_amd/csrc/kmws_resident.hip).

Reference: tests/utf8_ref.py validate_stream.  Routes and helpers: those of
tests/test_gpu_decoder_utf8.py (pageable bytes, a pinned buffer in place, ring +
flush, ring + submit / poll).  Every case asserts the verdicts equal the
reference's, that payload bytes and return codes equal those of the same feed
with the check off, and on the pinned CLIENT-mode route that the buffer is
untouched.

Geometry the layout cases aim at (kmws_resident.hip): a job's payload hulls
are numbered in 16-byte words; a workgroup runs rounds of 4096 words, 1024
lanes x 4 stripes of 1024 words, 64 words a wave; jobs of up to 1024 words
store write-through, larger ones release once; jobs of at least 2048 words are
split over min(4, words / 1024) parts at words * p / parts.  Checked jobs of
more than KMWS_RESIDENT_MAX_CHECKED_BYTES = 64 KiB launch, as every job over
256 KiB does -- so a checked part is one round of at most 4096 words, and the
longer lengths below check that the verdicts do not depend on the way."""
import random
import threading

import pytest

import test_gpu_decoder_utf8 as du
import utf8_ref as ref
from kuma_amd import kmws

gpu = pytest.mark.gpu

CP3, CP4 = du.CP3, du.CP4  # E2 82 AC, F0 9F 98 80
PINNED_ROUTES = ("pinned", "ring_flush", "ring_poll")
MAX_BYTES = 262144  # KMWS_RESIDENT_MAX_BYTES: a larger job launches
CHECKED_MAX_BYTES = 65536  # kResMaxBytesChecked (kmws_common.hpp): a larger checked job launches
MAX_PAYLOADS = 128  # KMWS_RESIDENT_MAX_PAYLOADS

_start = {}


@pytest.fixture(scope="module", autouse=True)
def _module_start():
    if kmws.device_count() > 0:
        _start.update(kmws.resident_utf8())
    yield


def callback_into(got):
    def cb(hdr, payload):
        b0 = (hdr.fin << 7) | (hdr.rsv1 << 6) | (hdr.rsv2 << 5) | (hdr.rsv3 << 4) | hdr.opcode
        got.append((b0, payload, hdr.utf8))
    return cb


def run_case(frames, masked=True, routes=du.ROUTES, groups=None, base=0, seed=1, want=None):
    """One connection's frames through the routes with the check on and off.
    groups: frames per feed (and, on ring_poll, per submit); None: one feed."""
    if want is None:
        want, _ = ref.validate_stream(frames)
    parts = du.wire_of(frames, masked, seed)
    wire = b"".join(parts)
    cuts, o, i = [], 0, 0
    for g in (groups or [len(parts)]):
        n = sum(len(p) for p in parts[i:i + g])
        cuts.append((o, n))
        o, i = o + n, i + g
    assert i == len(parts) and o == len(wire)
    for route in routes:
        rc_on, got_on, after_on = du.feed(route, wire, masked, True, cuts, base=base)
        rc_off, got_off, after_off = du.feed(route, wire, masked, False, cuts, base=base)
        assert [(b0, p) for b0, p, _ in got_on] == list(frames), route
        assert [g[2] for g in got_on] == want, (route, base, [g[2] for g in got_on], want)
        assert [(b0, p) for b0, p, _ in got_off] == list(frames), route
        assert all(g[2] == 0 for g in got_off), route
        assert rc_on == rc_off, route
        assert after_on == after_off, route
        if route == "pinned" and not masked:
            assert after_on == wire, "CLIENT mode: the pinned buffer is untouched"
    return want


# ---- 1. the path: checked jobs run on the grid ----

@gpu
def test_checked_feeds_stay_on_the_grid():
    rng = random.Random(11)
    pool = ref.TextPool(rng, 1 << 14)
    h = kmws.WSHandler(kmws.SERVER)
    h.setUtf8Check(True)
    got = []
    h.setFrameCallback(callback_into(got))
    payloads = [pool.take(rng, 4096) for _ in range(33)]
    wires = [du.frame_wire(0x81, p, bytes(rng.randrange(256) for _ in range(4))) for p in payloads]
    assert h.handleData(wires[32]) == kmws.WS_NOERR  # warm-up: claims the slot, brings the validating grid up
    assert kmws.resident_info()["thread_slot"] >= 0
    u0, j0 = kmws.resident_utf8(), kmws.resident_info()["jobs"]
    for w in wires[:32]:
        assert h.handleData(w) == kmws.WS_NOERR
    u1, j1 = kmws.resident_utf8(), kmws.resident_info()["jobs"]
    assert [(b0, p) for b0, p, _ in got] == [(0x81, payloads[32])] + [(0x81, p) for p in payloads[:32]]
    assert all(g[2] == ref.OK for g in got)
    # at most 2 of the 32 launched (a lease or idle relaunch never costs a job its place)
    assert u1["checked_jobs"] - u0["checked_jobs"] >= 30, (u0, u1)
    assert j1 - j0 >= 30, (j0, j1)
    assert u1["variant_switches"] - _start["variant_switches"] <= 1
    # check off, a fresh handler: unchecked jobs
    h2 = kmws.WSHandler(kmws.SERVER)
    got2 = []
    h2.setFrameCallback(callback_into(got2))
    for w in wires[:8]:
        assert h2.handleData(w) == kmws.WS_NOERR
    u2, j2 = kmws.resident_utf8(), kmws.resident_info()["jobs"]
    assert u2["checked_jobs"] == u1["checked_jobs"]
    assert j2 - j1 >= 6
    assert [g[2] for g in got2] == [0] * 8


# ---- 2. layout edges ----

LENGTHS = ([1, 15, 16, 17] + [1023, 1024, 1025] + [16383, 16384, 16385] + [16384 - 16, 16384 + 16] +
           [32768 - 16, 32768, 32768 + 16] + [50001] + [65535, 65536, 65537] + [98304, 196608, 262144] + [MAX_BYTES + 1])
BASES = [None, 0, 3, 17]  # None: pageable bytes (staged at an aligned offset); else the offset in the pinned buffers


def edge_text(n, phase):
    """n bytes of well-formed text: `phase` ASCII bytes, then E2 82 AC F0 9F 98
    80 repeated (7 bytes: against 16-byte words every straddle occurs), ASCII
    where a whole unit no longer fits."""
    phase = min(phase, n)
    unit = CP3 + CP4
    k = (n - phase) // len(unit)
    return b"a" * phase + unit * k + b"z" * (n - phase - k * len(unit))


def header_len(n):
    return 6 if n < 126 else (8 if n < 65536 else 14)


def boundary_words(words):
    """Word indices in the job at which something changes hands: the lane, the
    wave, the stripe and the round inside a part, and every part's first word."""
    parts = min(4, max(1, words // 1024))
    out = set()
    for p in range(parts):
        wb, we = words * p // parts, words * (p + 1) // parts
        if p:
            out.add(wb)
        for step in (1, 64, 1024, 4096):
            if wb + step < we:
                out.add(wb + step)
    return sorted(out)


def edge_positions(n, shift):
    """Payload positions next to each boundary the hull crosses (shift: the
    payload's first byte within its first 16-byte word), byte 0 and byte n - 1."""
    words = (shift + n + 15) // 16
    pos = {0, n - 1}
    for w in boundary_words(words):
        for q in (16 * w - shift - 1, 16 * w - shift):
            if 0 <= q < n:
                pos.add(q)
    return sorted(pos)


def test_grid_lengths_reach_every_part_count_and_stride():
    """CPU, on this file's own helpers: among the lengths that run on the grid
    (<= CHECKED_MAX_BYTES) are jobs of 1, 2, 3 and 4 parts, written through and
    released, with a lane, a wave and a stripe boundary inside a part -- the
    stripe one from a part of more than 1024 words, which an unaligned 64 KiB
    hull (4097 words, four parts) has."""
    parts, steps, wt = set(), set(), set()
    for n in (x for x in LENGTHS if x <= CHECKED_MAX_BYTES):
        for shift in (0, 3):
            words = (shift + n + 15) // 16
            parts.add(min(4, max(1, words // 1024)))
            wt.add(words <= 1024)
            steps |= {w for w in (1, 64, 1024) if w in boundary_words(words)}
    assert parts == {1, 2, 3, 4} and wt == {True, False} and steps == {1, 64, 1024}
    assert 4097 * 3 // 4 + 1024 in boundary_words(4097)


@gpu
@pytest.mark.parametrize("base", BASES, ids=lambda b: "bytes" if b is None else f"base{b}")
@pytest.mark.parametrize("n", LENGTHS)
def test_layout_edges(n, base):
    routes = ("bytes",) if base is None else PINNED_ROUTES
    if base is None:
        shift = 0
    else:
        shift = (du.pinned("read").data_ptr() + base + header_len(n)) % 16
        assert du.pinned("ring").data_ptr() % 16 == du.pinned("read").data_ptr() % 16
    u0 = kmws.resident_utf8()["checked_jobs"]
    for phase in range(4):
        assert run_case([(0x81, edge_text(n, phase))], routes=routes, base=base or 0) == [ref.OK]
    if n > CHECKED_MAX_BYTES:
        assert kmws.resident_utf8()["checked_jobs"] == u0, "over the checked jobs' byte limit: launched"
    else:
        assert kmws.resident_utf8()["checked_jobs"] > u0, "ran on the grid"
    clean = edge_text(n, n % 4)
    for q in edge_positions(n, shift):
        for byte in (0xFF, 0x80):
            p = bytearray(clean)
            if p[q] == byte:
                continue
            p[q] = byte
            run_case([(0x81, bytes(p))], routes=routes, base=base or 0)


# ---- 3. across the frames of one job ----

def fragments_of(body, n):
    """body cut into n non-empty fragments of 5 bytes (the rest in the last):
    with 7-byte units the code points straddle the cuts."""
    assert len(body) >= 5 * n
    cuts = [5 * i for i in range(n)] + [len(body)]
    return [body[cuts[i]:cuts[i + 1]] for i in range(n)]


@gpu
@pytest.mark.parametrize("n", [2, 17, 31, 32, 33, 128, 129])
def test_fragments_of_one_message_in_one_job(n):
    body = edge_text(5 * n + 9, 1)
    u0 = kmws.resident_utf8()["checked_jobs"]
    want = run_case(ref.message(fragments_of(body, n)))
    assert want == [ref.OK] * n
    u1 = kmws.resident_utf8()["checked_jobs"]
    if n > MAX_PAYLOADS:
        assert u1 == u0, "over the payload limit: launched"
    else:
        assert u1 > u0, "ran on the grid"
    # the FIN ends inside a code point -- with bytes of its own, and empty
    cut = edge_text(5 * n, 1) + CP4[:2]
    want = run_case(ref.message(fragments_of(cut, n)))
    assert want == [ref.OK] * (n - 1) + [ref.BAD]
    if n <= MAX_PAYLOADS:
        want = run_case(ref.message(fragments_of(cut, n) + [b""]))
        assert want == [ref.OK] * n + [ref.BAD]
    # one bad byte in the middle fragment: BAD there, AFTER_BAD behind it
    bad = bytearray(body)
    bad[5 * (n // 2) + 2] = 0xFF
    want = run_case(ref.message(fragments_of(bytes(bad), n)))
    assert want == [ref.OK] * (n // 2) + [ref.BAD] + [ref.AFTER_BAD] * (n - n // 2 - 1)


@gpu
@pytest.mark.parametrize("base", [0, 3, 17])
def test_one_read_of_sixteen_frames(base):
    """The job the grid exists for: 16 x 4 KiB text frames in one feed.  Behind
    their 8-byte headers the frames' hulls have 257 words (256 where a payload
    happens to start on a word), so the job has more than 4096 and each of its
    four parts more than 1024: the first words of a part's second stripe take
    their look-back from its first stripe's last wave."""
    frames = [(0x81, edge_text(4096, f % 4)) for f in range(16)]
    u0 = kmws.resident_utf8()["checked_jobs"]
    assert run_case(frames, routes=PINNED_ROUTES, base=base) == [ref.OK] * 16
    assert kmws.resident_utf8()["checked_jobs"] > u0, "ran on the grid"
    shifts = [(du.pinned("read").data_ptr() + base + 8 + f * (4096 + 8)) % 16 for f in range(16)]
    pre = [0]
    for sh in shifts:
        pre.append(pre[-1] + (sh + 4096 + 15) // 16)
    assert pre[-1] > 4096
    for w in boundary_words(pre[-1]):  # the bytes on both sides of every part, stripe, wave and lane hand-over
        if w in (1, 64):
            continue  # (inside the first frame: test_layout_edges)
        f = max(i for i in range(16) if pre[i] <= w)
        q, shift = w - pre[f], shifts[f]
        for pos in (16 * q - shift - 1, 16 * q - shift):
            if not 0 <= pos < 4096:
                continue
            for byte in (0xFF, 0x80):
                bad = bytearray(frames[f][1])
                bad[pos] = byte
                run_case(frames[:f] + [(0x81, bytes(bad))] + frames[f + 1:], routes=PINNED_ROUTES, base=base)


@gpu
def test_unchecked_payloads_in_a_checked_job():
    rng = random.Random(33)
    noise = lambda k: bytes(rng.randrange(256) for _ in range(k))
    t = edge_text(700, 2)
    frames = [(0x01, t[:333]), (0x89, noise(40)), (0x00, t[333:335]), (0x8A, b""), (0x80, t[335:]),
              (0x02, noise(900)), (0x00, noise(17)), (0x80, noise(1)),
              (0x41, noise(300)), (0x80, noise(30)),
              (0x81, t[:16])]
    want = run_case(frames)
    assert want == [1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 1]
    run_case(frames, masked=False)


@gpu
@pytest.mark.parametrize("groups", [[5], [3, 2], [1, 1, 1, 1, 1]])
def test_bad_then_after_bad_in_the_same_and_the_next_job(groups):
    t = edge_text(600, 0)
    frames = [(0x01, t[:100] + b"\xc0" + t[101:200]), (0x00, t[200:300]), (0x00, t[300:303]), (0x00, t[303:500]),
              (0x80, t[500:])]
    for masked in (True, False):
        want = run_case(frames, masked=masked, groups=groups)
        assert want == [ref.BAD] + [ref.AFTER_BAD] * 4


# ---- 4. key 0: CLIENT mode, unmasked text, checked in place ----

@gpu
def test_key_zero_is_checked_and_not_stored():
    rng = random.Random(44)
    pool = ref.TextPool(rng, 1 << 15)
    bad = bytearray(pool.take(rng, 5000))
    bad[4090] = 0xF8
    frames = [(0x81, pool.take(rng, 300)), (0x01, pool.take(rng, 20000)), (0x80, pool.take(rng, 5)),
              (0x81, bytes(bad)), (0x01, b"x\xe2\x82"), (0x80, b"")]
    u0 = kmws.resident_utf8()["checked_jobs"]
    want = run_case(frames, masked=False, routes=("pinned",), base=3)
    assert want == [1, 1, 1, 2, 1, 2]
    assert kmws.resident_utf8()["checked_jobs"] > u0


# ---- 5. two generations in flight ----

@gpu
@pytest.mark.parametrize("bad_first", [True, False])
def test_two_generations_in_flight(bad_first):
    """submit, submit, poll(wait): the second job of the slot finishes before
    the first generation's verdicts are read."""
    rng = random.Random(55)
    pool = ref.TextPool(rng, 1 << 14)
    ok = [(0x81, pool.take(rng, 1500)) for _ in range(3)]
    mixed = [(0x81, pool.take(rng, 1500)), (0x81, pool.take(rng, 700) + b"\xff" + pool.take(rng, 700)),
             (0x81, pool.take(rng, 90))]
    frames = mixed + ok if bad_first else ok + mixed
    want = run_case(frames, routes=("ring_poll",), groups=[3, 3])
    assert want == ([1, 2, 1, 1, 1, 1] if bad_first else [1, 1, 1, 1, 2, 1])


# ---- 6. threads ----

@gpu
def test_four_threads_of_checked_feeds():
    nthreads, nfeeds = 4, 200
    guard0 = kmws.resident_guard()["unowned_posts"]
    work = []
    for t in range(nthreads):
        rng = random.Random(600 + t)
        pool = ref.TextPool(rng, 1 << 15)
        msgs = []
        for _ in range(nfeeds):
            n = rng.randint(1024, 4096)
            if rng.random() < 0.3:
                frame = (0x82, bytes(rng.getrandbits(8) for _ in range(n)))
            else:
                p = bytearray(pool.take(rng, n))
                if rng.random() < 0.25:
                    p[rng.randrange(n)] = rng.choice((0xFF, 0xC0, 0x80, 0xF5))
                frame = (0x81, bytes(p))
            key = bytes(rng.getrandbits(8) for _ in range(4))
            msgs.append((frame, du.frame_wire(frame[0], frame[1], key), ref.validate_stream([frame])[0][0]))
        work.append(msgs)
    errors = []

    def run(t):
        try:
            h = kmws.WSHandler(kmws.SERVER)
            h.setUtf8Check(True)
            got = []
            h.setFrameCallback(callback_into(got))
            for _, wire, _ in work[t]:
                assert h.handleData(wire) == kmws.WS_NOERR
            assert [(b0, p) for b0, p, _ in got] == [f for f, _, _ in work[t]]
            assert [g[2] for g in got] == [w for _, _, w in work[t]]
        except BaseException as e:  # reported by the main thread
            errors.append((t, repr(e)[:300]))

    threads = [threading.Thread(target=run, args=(t,)) for t in range(nthreads)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    seen = {w for msgs in work for _, _, w in msgs}
    assert seen == {ref.NOT_TEXT, ref.OK, ref.BAD}
    assert kmws.resident_guard()["unowned_posts"] == guard0


@gpu
def test_variant_switches_over_the_module():
    """The validating instantiation is sticky: at most one incarnation was ever
    asked to leave for it."""
    assert kmws.resident_utf8()["variant_switches"] - _start["variant_switches"] <= 1
