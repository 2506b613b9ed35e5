"""The segmented-scan core (kuma_amd/csrc/kmws_stream_scan.hpp) on the device,
function by function, against a sequential fold: kuma_amd/probes/scan_probe.hip
instantiates block_scan_excl, scan_aggregates and the stream helpers with two
Ops in which every dropped prefix, swapped compose order or repeated element
shows (an interval of indices with a sticky "broken" flag: a multi-field struct
with a 64-bit count, and the same packed into one word).  The product monoids
absorb exactly those mistakes behind a stream's first frame.  Every comparison
is exact; every kernel runs one to three blocks."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 256  # kBlock: the lanes of a block


def round_aggregates() -> int:
    """kScanBlockFrames: the aggregates one round of scan_aggregates takes."""
    txt = open(os.path.join(ROOT, "kuma_amd", "csrc", "kmws_stream_scan.hpp")).read()
    return int(re.search(r"constexpr uint32_t kScanBlockFrames = (\d+);", txt).group(1))


R = round_aggregates()
GUARD = 64     # elements behind every output that must keep the fill pattern
FILL = 0xA7


# ---------------------------------------------------------------- the Ops, restated

class IntervalOp:
    """[lo, hi) with a count; a, then b joins only where a ends at b's start."""
    name = "interval"
    dtype = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("ident", "<u4"), ("broken", "<u4"), ("count", "<u8")])
    identity = (0xFFFFFFFF, 0xFFFFFFFF, 1, 0, 0)

    @staticmethod
    def elem(b, w=1):
        return (b, b + 1, 0, 0, w)

    @staticmethod
    def compose(a, b):
        if a[2]:
            return b
        if b[2]:
            return a
        return (a[0], b[1], 0, a[3] | b[3] | int(a[1] != b[0]), (a[4] + b[4]) & (2**64 - 1))

    @staticmethod
    def span(lo, hi, w=1):
        return IntervalOp.identity if lo == hi else (lo, hi, 0, 0, (hi - lo) * w)


class WordOp:
    """The same in one word: lo in bits 0-15, hi in bits 16-31; the count is not kept."""
    name = "word"
    dtype = np.dtype("<u4")
    identity = 0xFFFFFFFF
    poison = 0xFFFEFFFE

    @staticmethod
    def elem(b, w=1):
        return b | (b + 1) << 16

    @staticmethod
    def compose(a, b):
        if a == WordOp.identity:
            return b
        if b == WordOp.identity:
            return a
        if a == WordOp.poison or b == WordOp.poison or (a >> 16) != (b & 0xFFFF):
            return WordOp.poison
        return (a & 0xFFFF) | (b & 0xFFFF0000)

    @staticmethod
    def span(lo, hi, w=1):
        return WordOp.identity if lo == hi else lo | hi << 16


OPS = {"interval": IntervalOp, "word": WordOp}


def fold_excl(op, elems):
    """-> (the composition of elems[:k] for every k < len, that of all), one compose at a time."""
    run, pre = op.identity, []
    for e in elems:
        pre.append(run)
        run = op.compose(run, e)
    return pre, run


def test_the_ops_show_every_scan_mistake():
    """The restated Ops themselves: a skipped, a repeated and a swapped element each leave a mark."""
    for op in OPS.values():
        e = [op.elem(b) for b in range(5)]
        good = fold_excl(op, e)[1]
        assert good == op.span(0, 5) and good != op.identity
        for wrong in (e[:2] + e[3:], e[:3] + e[2:], [e[1], e[0]] + e[2:], e[1:]):
            assert fold_excl(op, wrong)[1] != good
        assert fold_excl(op, [op.identity, e[0], op.identity, e[1]])[1] == op.span(0, 2)


# ---------------------------------------------------------------- the probe library

@functools.lru_cache(maxsize=None)
def probe():
    from kuma_amd import build as kb
    assert os.path.exists(kb.SCAN_PROBE_LIB), "run __graft_entry__.build()"
    L = C.CDLL(kb.SCAN_PROBE_LIB)
    vp, u32 = C.c_void_p, C.c_uint32
    for name in ("interval", "word"):
        getattr(L, "kmws_probe_scan_aggs_" + name).argtypes = [vp, vp, u32, vp, vp, vp, vp]
        getattr(L, "kmws_probe_block_scan_" + name).argtypes = [vp, u32, vp, vp, vp]
    L.kmws_probe_streams.argtypes = [vp, u32, u32, vp, vp, vp, vp]
    L.kmws_probe_first_bad.argtypes = [vp, u32, u32, u32, vp, vp]
    L.kmws_probe_round.restype = L.kmws_probe_block.restype = u32
    assert (L.kmws_probe_round(), L.kmws_probe_block()) == (R, BLOCK)
    return L


def to_dev(values, dtype):
    import torch as T
    a = np.array(values, dtype=dtype).reshape(-1)
    return T.from_numpy(a.view(np.uint8).copy()).cuda()


def filled(count, dtype):
    """count + GUARD elements of the fill pattern on the device."""
    import torch as T
    return T.full(((count + GUARD) * np.dtype(dtype).itemsize,), FILL, dtype=T.uint8, device="cuda")


def from_dev(t, count, dtype):
    """-> the first count elements as a list of Python values; the rest must be untouched."""
    raw = t.cpu().numpy()
    size = np.dtype(dtype).itemsize
    assert (raw[count * size:] == FILL).all(), "an output was written past its end"
    return raw[:count * size].view(dtype).tolist()


def stream_handle():
    import torch as T
    return int(T.cuda.current_stream().cuda_stream)


def mismatches(got, want):
    bad = [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
    return [(k, got[k], want[k]) for k in bad[:5]]


# ---------------------------------------------------------------- scan_aggregates

NAGG = [1, 3, 4, 5, 255, 256, 257, R - 1, R, R + 1, R + 5, R + 257, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R + 7]
BIG = (1 << 33) + 1  # a count whose sum needs the 64-bit field's high half


def run_scan_aggs(op, elems, bits):
    import torch as T
    nagg = len(elems)
    d_aggs, d_bits = to_dev(elems, op.dtype), to_dev(bits, np.uint32)
    pre, total, status = filled(nagg, op.dtype), filled(BLOCK, op.dtype), filled(1, np.uint32)
    rc = getattr(probe(), "kmws_probe_scan_aggs_" + op.name)(d_aggs.data_ptr(), d_bits.data_ptr(), nagg, pre.data_ptr(),
                                                             total.data_ptr(), status.data_ptr(), stream_handle())
    assert rc == 0
    T.cuda.synchronize()
    return from_dev(pre, nagg, op.dtype), from_dev(total, BLOCK, op.dtype), from_dev(status, 1, np.uint32)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("nagg", NAGG)
@pytest.mark.parametrize("op", list(OPS.values()), ids=list(OPS))
def test_scan_aggregates(op, nagg):
    """pre[b] is exactly [0, b) for every b < nagg and every lane gets [0, nagg)
    back, in one, two, three and four rounds; nothing is stored at or past nagg;
    a status bit beside one aggregate reaches the block's OR wherever it lies."""
    elems = [op.elem(b) for b in range(nagg)]
    want_pre, want_total = fold_excl(op, elems)
    assert want_pre == [op.span(0, b) for b in range(nagg)] and want_total == op.span(0, nagg)  # the fold's own answer
    pre, total, status = run_scan_aggs(op, elems, [0] * nagg)
    assert not mismatches(pre, want_pre), mismatches(pre, want_pre)
    assert total == [want_total] * BLOCK, mismatches(total, [want_total] * BLOCK)
    assert status == 0
    # one flagged aggregate in each position in turn; the counts now past 2^32
    elems = [op.elem(b, BIG) for b in range(nagg)]
    want_pre, want_total = fold_excl(op, elems)
    assert want_total == op.span(0, nagg, BIG)
    for where in sorted({0, nagg - 1} | {p for p in (R + 4, 2 * R) if p < nagg}):
        bits = [0] * nagg
        bits[where] = 0x10
        pre, total, status = run_scan_aggs(op, elems, bits)
        assert status == 1, where
        assert not mismatches(pre, want_pre), (where, mismatches(pre, want_pre))
        assert total == [want_total] * BLOCK, where


# ---------------------------------------------------------------- block_scan_excl

@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 255, 256])
@pytest.mark.parametrize("op", list(OPS.values()), ids=list(OPS))
def test_block_scan_excl(op, m):
    """Three blocks whose first m lanes hold elements and the rest the identity:
    every lane's exclusive value and the total every lane is given."""
    import torch as T
    nblocks = 3
    elems = []
    for blk in range(nblocks):
        base = 1000 * blk + 7
        elems += [op.elem(base + t, BIG) if t < m else op.identity for t in range(BLOCK)]
    want_excl, want_total = [], []
    for blk in range(nblocks):
        base = 1000 * blk + 7
        pre, tot = fold_excl(op, elems[blk * BLOCK:(blk + 1) * BLOCK])
        assert pre == [op.span(base, base + min(t, m), BIG) for t in range(BLOCK)] and tot == op.span(base, base + m, BIG)
        want_excl += pre
        want_total += [tot] * BLOCK
    d_elems = to_dev(elems, op.dtype)
    excl, total = filled(nblocks * BLOCK, op.dtype), filled(nblocks * BLOCK, op.dtype)
    rc = getattr(probe(), "kmws_probe_block_scan_" + op.name)(d_elems.data_ptr(), nblocks, excl.data_ptr(),
                                                              total.data_ptr(), stream_handle())
    assert rc == 0
    T.cuda.synchronize()
    excl, total = from_dev(excl, nblocks * BLOCK, op.dtype), from_dev(total, nblocks * BLOCK, op.dtype)
    assert not mismatches(excl, want_excl), mismatches(excl, want_excl)
    assert not mismatches(total, want_total), mismatches(total, want_total)


# ---------------------------------------------------------------- stream_of, LaneStreams

STREAM_N = [1, 4, 5, R - 1, R, R + 1, 2 * R + 1]
STREAM_LAYOUTS = ["null", "stream_per_frame", "empty_runs", "inside_lanes", "more_streams_than_frames"]


def stream_layout(kind, n):
    """-> stream_first (ns + 1 entries), or None."""
    if kind == "null":
        return None
    if kind == "stream_per_frame":
        return list(range(n + 1))
    if kind == "empty_runs":  # runs of empty streams first, in the middle and last
        a, b = n // 3, 2 * n // 3
        return [0, 0, 0, a, a, a, b, n, n, n]
    if kind == "inside_lanes":  # a lane holds frames 4j .. 4j + 3: streams begin at its 2nd, 3rd and 4th, some at two
        starts = {0}
        for j in range((n + 3) // 4):
            starts.add(4 * j + 1 + j % 3)
            if j % 7 == 0:
                starts |= {4 * j + 1, 4 * j + 3}
        return sorted(p for p in starts if p < n) + [n]
    if kind == "more_streams_than_frames":  # every frame a stream, empty ones first, in the middle and last
        return sorted(list(range(n + 1)) + [0, n // 2, n // 2, n, n])
    raise ValueError(kind)


def test_stream_layouts_are_what_they_claim():
    """CPU: ascending from 0 to n; the named features are there at every n that has room for them."""
    for n in STREAM_N:
        for kind in STREAM_LAYOUTS[1:]:
            f = stream_layout(kind, n)
            assert f[0] == 0 and f[-1] == n and all(a <= b for a, b in zip(f, f[1:])), (kind, n)
        assert len(stream_layout("more_streams_than_frames", n)) - 1 == n + 5
        if n >= 16:
            assert {p % 4 for p in stream_layout("inside_lanes", n)[1:-1]} == {1, 2, 3}
            lanes = [p // 4 for p in stream_layout("inside_lanes", n)[1:-1]]
            assert len(lanes) > len(set(lanes))  # a lane with two stream starts


@pytest.mark.gpu
@pytest.mark.parametrize("n", STREAM_N)
@pytest.mark.parametrize("kind", STREAM_LAYOUTS)
def test_stream_of_and_lane_streams(kind, n):
    import torch as T
    first = stream_layout(kind, n)
    ns = 1 if first is None else len(first) - 1
    f = np.array([0, n] if first is None else first, dtype=np.int64)
    i = np.arange(n)
    s = np.searchsorted(f[:ns], i, "right") - 1
    want_edges = ((f[s] == i) * 1 + (f[s + 1] == i + 1) * 2).tolist()
    d_first = None if first is None else to_dev(first, np.uint32)
    outs = [filled(n, np.uint32), filled(n, np.uint32), filled(n, np.uint8)]
    rc = probe().kmws_probe_streams(None if first is None else d_first.data_ptr(), ns, n, *[o.data_ptr() for o in outs],
                                    stream_handle())
    assert rc == 0
    T.cuda.synchronize()
    direct, lane, edges = (from_dev(o, n, dt) for o, dt in zip(outs, (np.uint32, np.uint32, np.uint8)))
    assert not mismatches(direct, s.tolist()), mismatches(direct, s.tolist())
    assert not mismatches(lane, s.tolist()), mismatches(lane, s.tolist())
    assert not mismatches(edges, want_edges), mismatches(edges, want_edges)


# ---------------------------------------------------------------- stream_first_bad

def first_bad_contract(first, ns, n, x):
    """[0] == 0, ascending, [ns] == n; nothing to say without an array or past ns."""
    if first is None or x > ns:
        return False
    return (x == 0 and first[0] != 0) or (x == ns and first[ns] != n) or (x < ns and first[x] > first[x + 1])


def first_bad_cases():
    """The malformed arrays of the entries' test_malformed_stream_first_sets_status_bit_1
    ([1, 3, 5], [0, 4, 3], [0, 3, 4], [0, 3, 6] for five frames) grown to R + 3
    entries, the descending pair at both ends and on either side of entry R."""
    ns = R + 2
    good = [k // 2 * 2 for k in range(ns + 1)]  # ascending, every other stream empty
    n = good[ns]
    cases = [("good", good, n), ("null", None, n)]

    def edit(name, at, value):
        f = list(good)
        f[at] = value
        cases.append((name, f, n))

    edit("first_not_0", 0, 1)
    edit("last_below_n", ns, n - 1)
    edit("last_above_n", ns, n + 1)
    for at in (1, R - 1, R, R + 1, ns - 1):
        edit(f"descending_at_{at}", at, good[at + 1] + 1)
    return ns, cases


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(10))
def test_stream_first_bad(case):
    import torch as T
    ns, cases = first_bad_cases()
    assert len(cases) == 10
    name, first, n = cases[case]
    count = ns + 1 + 8  # past ns too: nothing there is an entry
    want = [int(first_bad_contract(first, ns, n, x)) for x in range(count)]
    if name not in ("good", "null"):
        assert 1 <= sum(want) <= 2, (name, sum(want))  # a raised entry also stands above its successor
    else:
        assert sum(want) == 0
    d_first = None if first is None else to_dev(first, np.uint32)
    bad = filled(count, np.uint8)
    rc = probe().kmws_probe_first_bad(None if first is None else d_first.data_ptr(), ns, n, count, bad.data_ptr(),
                                      stream_handle())
    assert rc == 0
    T.cuda.synchronize()
    got = from_dev(bad, count, np.uint8)
    assert not mismatches(got, want), (name, mismatches(got, want))
