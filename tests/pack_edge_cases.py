"""Deterministic edge cases for the encode / gather copy kernels of
kuma_amd/csrc/kmws_pack.hip, and a small geometry model that says which
structural edge a batch lands on.  Plain numpy: no torch, no GPU.

A case is a list of REGION sizes (a region = header + payload for encode, the
payload alone for a gather) laid out back to back in the output, so one list
gives the same output geometry to both templates of the copy kernels:
`build(headers=True)` turns every region into a frame whose header + payload
has that size, `build(headers=False)` into a payload of that size.  Every
builder returns (src, offs, lens, flags, keys).

The model restates from the kernel source only what classifies a batch: the
region starts, the chunk map and frame counts of the chunk form, the boundary
words chunk_copy_kernel lists, and frame_words / the three-region test of the
unit form's prologue.  tests/test_pack_edge_cases.py checks each case's
claimed property against it (and the constants below against the source);
tests/test_gpu_pack_edges.py runs the cases on the device.
"""
import zlib

import numpy as np

# The structural constants of kmws_pack.hip / kmws_common.hpp the cases are
# aimed at (guarded by test_constants_match_the_kernel_source).
kChunkBytes = 4096       # chunk form: one wave per 4 KiB of output
kChunkFrames = 64        # a chunk's frame table; more frames -> chunk_dense_kernel
kLineBytes = 64          # unit form: ownership granule
kUnitWords = 256         # unit form: 16-byte words per wave unit
kUnitAlign = 64          # unit bases are aligned to this many words (1 KiB)
kScanTile = 2048         # frames per scan tile
kBlock = 256             # frames per row (prologue / chunk_map block)
kChunkFormBelow = 16384  # dst_cap // n below this: chunk form, else unit form
CONSTANTS = dict(kChunkBytes=kChunkBytes, kChunkFrames=kChunkFrames, kLineBytes=kLineBytes,
                 kUnitWords=kUnitWords, kUnitAlign=kUnitAlign, kScanTile=kScanTile, kBlock=kBlock,
                 kChunkFormBelow=kChunkFormBelow)
kLineWords = kLineBytes // 16
kChunkWords = kChunkBytes // 16

FIN_BINARY = 0x82
MASK_BIT = 0x100


def header_len(length, mask):
    """Bytes of encodeFrameHeader for a payload of `length` bytes."""
    length = np.asarray(length, dtype=np.int64)
    return np.where(length <= 125, 2, np.where(length <= 0xFFFF, 4, 10)) + 4 * np.asarray(mask, dtype=np.int64)


def use_chunks(n, cap):
    """The host's form rule (copy_uses_chunks in kmws_workspace.hpp)."""
    return n > 0 and cap // n < kChunkFormBelow


def _ceil_div(a, b):
    return -(-a // b)


# ------------------------------ the model ------------------------------
class Geometry:
    """Output geometry of a batch: region r0, payload start p0, region end r1."""

    def __init__(self, offs, lens, flags, headers):
        self.headers = bool(headers)
        self.n = len(lens)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.offs = np.asarray(offs, dtype=np.int64)
        mask = (np.asarray(flags, dtype=np.int64) >> 8) & 1
        hdr = header_len(self.lens, mask) if headers else np.zeros(self.n, np.int64)
        size = hdr + self.lens
        ends = np.cumsum(size)
        self.r0 = ends - size
        self.p0 = self.r0 + hdr
        self.r1 = ends
        self.total = int(ends[-1]) if self.n else 0
        # the funnel shift of a payload's interior words: (source - output) mod 16
        self.delta = (self.offs - self.p0) & 15

    # ---- chunk form ----
    @property
    def nch(self):
        return _ceil_div(self.total, kChunkBytes)

    def chunk_map(self):
        """cmap[c]: the last frame whose region starts at or before byte 4096 c."""
        c = np.arange(self.nch, dtype=np.int64) * kChunkBytes
        return np.searchsorted(self.r0, c, side="right") - 1

    def chunk_nfr(self):
        """Frames in chunk c's table: cmap[c+1] - cmap[c] + 1, n - 1 standing in past the last chunk."""
        cm = self.chunk_map()
        if len(cm) == 0:
            return cm
        nxt =np.concatenate([cm[1:], [self.n - 1]])
        return nxt - cm + 1

    def dense_chunks(self):
        return int(np.sum(self.chunk_nfr() > kChunkFrames))

    def chunk_words(self, c):
        """Pass 1 of chunk_copy_kernel for chunk c (nfr <= 64): per word k of the
        chunk its frame, and whether it is live, interior to one payload, takes
        its second source word from the neighbour lane (nb), from the lane's one
        extra load (ex), or is listed as a boundary word (slow)."""
        A0 = c * kChunkBytes
        k = np.arange(kChunkWords)
        a = A0 + 16 * k
        fr = np.searchsorted(self.r0, a, side="right") - 1
        trel = min(self.total - A0, kChunkBytes)
        live = 16 * k < trel
        inner = live & (a >= self.p0[fr]) & (a + 16 <= self.r1[fr])
        delta = self.delta[fr]
        nb = (delta == 0) | ((a + 32 <= self.r1[fr]) & (k != kChunkWords - 1))
        need = (inner & ~nb).reshape(4, 64)          # [round, lane]
        first = np.cumsum(need, axis=0) == 1
        ex = (need & first).reshape(-1)              # the lane's first word that needs it
        fast = inner & (nb | ex)
        slow = live & ~fast
        return dict(frame=fr, live=live, inner=inner, delta=delta, nb=nb, ex=ex, slow=slow)

    def chunk_boundary_words(self, c):
        """Words of chunk c that chunk_copy_kernel composes byte by byte (its nslow)."""
        return int(self.chunk_words(c)["slow"].sum())

    def chunk_non_interior_words(self, c):
        """Live words of chunk c that are not interior to one payload."""
        w = self.chunk_words(c)
        return int((w["live"] & ~w["inner"]).sum())

    # ---- unit form ----
    def frame_words(self, clip=False):
        """frame_words(): owned words [olo, ohi), interior [ilo, ihi), first unit
        base b0 and the unit count, per frame (word = 16 output bytes).  The
        prologue computes them unclipped; the copy waves clip at the total."""
        olo = kLineWords * _ceil_div(self.r0, kLineBytes)
        ohi = kLineWords * _ceil_div(self.r1, kLineBytes)
        if clip:
            ohi = np.minimum(ohi, _ceil_div(self.total, 16))
        ohi = np.maximum(ohi, olo)
        ilo = np.maximum(_ceil_div(self.p0, 16), olo)
        ihi = np.minimum(self.r1 >> 4, ohi)
        ilo = np.minimum(ilo, ohi)
        ihi = np.maximum(ihi, ilo)
        b0 = olo & ~(kUnitAlign - 1)
        units = np.where(ohi > olo, _ceil_div(ohi - b0, kUnitWords), 0)
        return dict(olo=olo, ohi=ohi, ilo=ilo, ihi=ihi, b0=b0, units=units)

    def regions_in_word(self, word):
        """Regions with at least one byte in output word `word`."""
        a = 16 * int(word)
        return int(np.sum((self.r0 < a + 16) & (self.r1 > a)))

    def third_words(self, f):
        """row_prologue's `third` bits of frame f as {edge position q: word}: the
        edge words a third region reaches into, composed by compose_word_bytes.
        q < head_f: the head word; q = head_f + i: tail position i."""
        w = self.frame_words()
        olo, ohi, ilo, ihi = (int(w[x][f]) for x in ("olo", "ohi", "ilo", "ihi"))
        head_f, ntail = ilo - olo, ohi - ihi
        out = {}
        if head_f and self.r1[f] < 16 * olo + 16 and f + 1 < self.n:
            out[0] = olo
        if f + 1 < self.n:
            for i in range(min(ntail, kLineWords)):
                a = 16 * (ihi + i)
                if self.r0[f + 1] < a + 16 and self.r1[f + 1] < a + 16 and f + 2 < self.n:
                    out[head_f + i] = ihi + i
        return out, head_f


# ------------------------------ builders ------------------------------
def frames_from_regions(regions, headers, prefer_mask=1):
    """(lens, flags) of frames whose regions have the given sizes.  With headers a
    region is header + payload: the mask bit is `prefer_mask` where a frame of
    that size exists with it, else the other one."""
    regions = [int(r) for r in regions]
    if not headers:
        return np.array(regions, dtype=np.int64), np.full(len(regions), FIN_BINARY | MASK_BIT, dtype=np.uint32)
    lens, flags = [], []
    for k, R in enumerate(regions):
        pm = prefer_mask if np.isscalar(prefer_mask) else prefer_mask[k]
        for mask in (int(pm), 1 - int(pm)):
            fit = [R - h - 4 * mask for h in (2, 4, 10)]
            fit = [L for L in fit if L >= 0 and int(header_len(L, mask)) + L == R]
            if fit:
                lens.append(fit[0])
                flags.append(FIN_BINARY | (MASK_BIT if mask else 0))
                break
        else:
            raise ValueError(f"no frame has a region of {R} bytes")
    return np.array(lens, dtype=np.int64), np.array(flags, dtype=np.uint32)


def layout_source(name, lens, phases=None):
    """A source arena holding the payloads in order, payload k at a byte phase
    (offset mod 16) of phases[k] (seeded random where None), with gaps of 0-2
    words between them; 64 spare bytes at the end.  Keys: every 7th is 0."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = len(lens)
    ph = rng.integers(0, 16, size=n) if phases is None else np.asarray(phases, dtype=np.int64)
    gap = rng.integers(0, 3, size=n) * 16
    offs = np.zeros(n, dtype=np.int64)
    cur = 0
    for k in range(n):
        offs[k] = cur + int(gap[k]) + int(ph[k])
        cur = (int(offs[k]) + int(lens[k]) + 15) // 16 * 16
    src = rng.integers(0, 256, size=cur + 64, dtype=np.uint8)
    keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[::7] = 0
    return src, offs.astype(np.uint64), keys


def from_regions(name, regions, headers, deltas=None, prefer_mask=1):
    """The batch of a region list; deltas[k] (None: random) = the funnel shift
    (source - output) mod 16 of frame k's payload."""
    lens, flags = frames_from_regions(regions, headers, prefer_mask)
    phases = None
    if deltas is not None:
        g = Geometry(np.zeros(len(lens)), lens, flags, headers)
        phases = (g.p0 + np.asarray(deltas, dtype=np.int64)) & 15
    src, offs, keys = layout_source(f"{name}-{int(headers)}", lens, phases)
    return src, offs, lens, flags, keys


class Case:
    """name; regions(headers) -> (region sizes, deltas or None); check(g) asserts
    the property the name claims on the model; forms the entries it applies to."""

    def __init__(self, name, group, regions, check, encode=True, gather=True):
        self.name, self.group, self._regions, self.check = name, group, regions, check
        self.encode, self.gather = encode, gather

    def variants(self):
        return [h for h, on in ((True, self.encode), (False, self.gather)) if on]

    def build(self, headers):
        regions, deltas = self._regions(headers)
        return from_regions(self.name, regions, headers, deltas)

    def geometry(self, headers):
        src, offs, lens, flags, keys = self.build(headers)
        return Geometry(offs, lens, flags, headers)


CASES = {}


def _case(name, group, **kw):
    def reg(fn):
        def regions(headers):
            out = fn(headers)
            return out if isinstance(out, tuple) else (out, None)
        CASES[name] = Case(name, group, regions, kw.pop("check"), **kw)
        return fn
    return reg


# ---- chunk form ----
def _check_nfr_64_65(g):
    nfr = g.chunk_nfr()
    assert any(nfr[c] == kChunkFrames and nfr[c + 1] == kChunkFrames + 1 for c in range(len(nfr) - 1)), nfr
    assert any(nfr[c] == kChunkFrames + 1 and nfr[c + 1] == kChunkFrames for c in range(len(nfr) - 1)), nfr
    assert g.dense_chunks() == 2


@_case("chunk_nfr_64_65", "chunk", check=_check_nfr_64_65)
def _(headers):
    # 63 frames inside a chunk + the one holding the next chunk's first byte = 64
    # (the table is full); 64 inside + 1 = 65 (dense); and back again
    full = [64] * 62 + [128]
    dense = [64] * 64
    return [8192] + full + dense + dense + full + [5000]


# boundary-word counts: a shifter region, X small unaligned regions, one filler,
# with one funnel shift for all; (shifter, X, small size, delta) found with the
# model for each template (test_pack_edge_cases asserts the count)
_BOUNDARY_PARAMS = {
    (64, True): (11, 31, 32, 0), (65, True): (27, 31, 32, 0),
    (80, True): (11, 39, 32, 0), (81, True): (27, 39, 32, 0),
    # payload only: one boundary word per small region, the rest from lanes whose
    # words need the extra load more than once (delta != 0)
    (64, False): (6, 47, 32, 5), (65, False): (33, 47, 32, 5),
    (80, False): (6, 55, 32, 5), (81, False): (33, 55, 32, 5),
}


def _boundary_regions(target, headers, params=None):
    s, x, small, delta = params or _BOUNDARY_PARAMS[(target, headers)]
    regions = [kChunkBytes, s] + [small] * x  # chunk 1 = the shifter, the small regions, the filler's start
    regions += [2 * kChunkBytes - sum(regions) + 1000, 3000]
    return regions, [delta] * len(regions)


def _check_boundary(target):
    def check(g):
        assert g.chunk_nfr()[1] <= kChunkFrames, g.chunk_nfr()
        assert g.chunk_boundary_words(1) == target, g.chunk_boundary_words(1)
    return check


def _boundary_case(target):
    @_case(f"chunk_boundary_words_{target}", "chunk", check=_check_boundary(target))
    def _(headers):
        return _boundary_regions(target, headers)


for _t in (64, 65, 80, 81):
    _boundary_case(_t)


def _check_payload_end(d):
    def check(g):
        e = g.r1[g.lens > 0]
        assert np.any((e > kChunkBytes) & ((e - d) % kChunkBytes == 0)), e
    return check


def _payload_end_case(tag, d):
    @_case(f"chunk_payload_end_edge_{tag}", "chunk", check=_check_payload_end(d))
    def _(headers):
        return [1500, 2 * kChunkBytes - 1500 + d, 900, kChunkBytes - 900, 700, 4000]


_payload_end_case("minus1", -1)
_payload_end_case("exact", 0)
_payload_end_case("plus1", 1)


def _check_lane63(g):
    seen = set()
    for c in range(g.nch):
        if g.chunk_nfr()[c] > kChunkFrames:
            continue
        w = g.chunk_words(c)
        last = kChunkWords - 1
        fr = w["frame"][last]
        if w["inner"][last] and w["delta"][last] and 16 * (c * kChunkWords + last) + 32 <= g.r1[fr] and w["ex"][last]:
            seen.add("lane63_extra")      # only the `lane != 63` term sends it to the extra load
        if w["inner"][63] and w["inner"][64] and w["delta"][63] and w["nb"][63] and w["frame"][63] == w["frame"][64]:
            seen.add("lane63_to_lane0")   # second source word from lane 0 of the next round
        if w["inner"].all() and not w["delta"][0]:
            seen.add("aligned")           # delta == 0: no second source word at all
        if np.any(w["ex"][:last]):
            seen.add("payload_last_word")  # a payload's last interior word: the extra load
    assert seen == {"lane63_extra", "lane63_to_lane0", "aligned", "payload_last_word"}, seen


@_case("chunk_lane63_extra_load", "chunk", check=_check_lane63)
def _(headers):
    regions = [3 * kChunkBytes + 100, 2 * kChunkBytes + 700, 1300, 3 * kChunkBytes - 2100, 900]
    return regions, [5, 0, 11, 9, 3]


def _check_total(mod, rem):
    def check(g):
        assert g.total % mod == rem, g.total
        if mod == 16:
            assert g.total % kChunkBytes != rem
    return check


def _total_case(tag, mod, rem):
    @_case(f"chunk_total_{tag}", "chunk", check=_check_total(mod, rem))
    def _(headers):
        regions = [700, 5000, 333, 2500, 90]
        want = 3 * kChunkBytes if mod == kChunkBytes else 2 * kChunkBytes + 16 * 37 + rem
        return regions + [want - sum(regions)]


_total_case("mod4096_0", kChunkBytes, 0)
_total_case("mod16_0", 16, 0)
_total_case("mod16_1", 16, 1)


# ---- gather batches with empty regions ----
def _runs_of_empties(g):
    z = np.concatenate([[0], (g.lens == 0).astype(np.int64), [0]])
    d = np.diff(z)
    return list(zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]))  # [first, past)


def _check_empty_run_chunk_start(g):
    runs = [(a, b) for a, b in _runs_of_empties(g) if b - a == 70]
    # one run sits exactly on a chunk start, one just before a chunk start that
    # the payload after it crosses
    assert any(g.r0[a] % kChunkBytes == 0 and g.r0[a] > 0 for a, b in runs)
    assert any(g.r0[a] % kChunkBytes == kChunkBytes - 6 and g.lens[b] > 6 for a, b in runs)
    cm = g.chunk_map()
    assert np.any(np.diff(cm) > 70)


@_case("empty_run_across_chunk_start", "empty", encode=False, check=_check_empty_run_chunk_start)
def _(headers):
    return [4096] + [0] * 70 + [4090] + [0] * 70 + [3000, 20, 0, 0, 7000]


def _check_empty_tile(g):
    assert g.n <= 4097 and np.all(g.lens[kScanTile:2 * kScanTile] == 0)
    (a, b), = [(a, b) for a, b in _runs_of_empties(g) if b - a >= kScanTile]
    assert b - a == 2100 and a > 0 and b < g.n and g.lens[a - 1] > 0 and g.lens[b] > 0


@_case("empty_whole_scan_tile", "empty", encode=False, check=_check_empty_tile)
def _(headers):
    rng = np.random.default_rng(11)
    return list(rng.integers(1, 200, size=1996)) + [0] * 2100 + [5000]


def _check_empty_trailing(g):
    assert np.all(g.lens[-300:] == 0) and g.lens[-301] > 0
    assert g.chunk_nfr()[-1] > 300  # f1 = n - 1: the last chunk's table would hold them all


@_case("empty_trailing_300", "empty", encode=False, check=_check_empty_trailing)
def _(headers):
    return [3000, 0, 41, 6000, 17] + [0] * 300


def _check_empty_all(g):
    assert g.n == 300 and g.total == 0 and g.nch == 0


@_case("empty_all_300", "empty", encode=False, check=_check_empty_all)
def _(headers):
    return [0] * 300


# ---- unit form ----
def _check_region_end(d):
    def check(g):
        w = g.frame_words()
        assert np.any((w["units"][:-1] > 0) & (g.r1[:-1] % kLineBytes == d % kLineBytes) & (g.r1[:-1] > 1024))
    return check


def _region_end_case(tag, d):
    @_case(f"unit_region_end_granule_{tag}", "unit", check=_check_region_end(d))
    def _(headers):
        return [700, 64 * 40 - 700 + d, 1300, 64 * 90 - 64 * 40 - 1300, 2000 + d, 500]


_region_end_case("minus1", -1)
_region_end_case("exact", 0)
_region_end_case("plus1", 1)


def _check_zero_granule(g):
    u = g.frame_words()["units"]
    assert list(u[1:4]) == [0, 0, 0] and u[0] >= 2 and u[4] >= 2, u
    assert np.all(g.lens[1:4] > 0)
    assert np.all(g.r0[1:4] // kLineBytes == (g.r1[1:4] - 1) // kLineBytes)  # inside one granule


@_case("unit_zero_granule_frames", "unit", check=_check_zero_granule)
def _(headers):
    return [5001, 10, 20, 9, 6000, 8, 3000]


def _check_third(position):
    def check(g):
        hit = False
        for f in range(g.n):
            third, head_f = g.third_words(f)
            if position == "head":
                ok = head_f and 0 in third and g.regions_in_word(third[0]) >= 3
            else:
                q = head_f + position
                ok = q in third and g.regions_in_word(third[q]) >= 3 and g.frame_words()["units"][f] >= 1
            hit |= bool(ok)
        assert hit
    return check


@_case("unit_third_region_head", "unit", gather=False, check=_check_third("head"))
def _(headers):
    # frame 1 starts on a granule and ends inside its head word; so does frame 2
    return [4096, 6, 6, 3000, 64 * 3 - 22 + 6, 6, 7, 1000]


def _third_tail_case(i):
    @_case(f"unit_third_region_tail_{i}", "unit", check=_check_third(i))
    def _(headers):
        # frame 0 ends 4 bytes into a granule; frame 1 ends inside tail word i;
        # frames 2 and 3 follow inside the same word
        return [64 * 50 + 4, 16 * i + 4, 6, 3000, 500]


for _i in range(4):
    _third_tail_case(_i)


def _check_olo_b0(want):
    def check(g):
        w = g.frame_words()
        assert np.any((w["olo"] - w["b0"] == want) & (w["units"] >= 2))
    return check


@_case("unit_olo_minus_b0_0", "unit", check=_check_olo_b0(0))
def _(headers):
    return [3 * 1024 - 30, 6000, 12 * 1024 - (3 * 1024 - 30) - 6000, 4100, 100]  # frames 1 and 3


@_case("unit_olo_minus_b0_60", "unit", check=_check_olo_b0(kUnitAlign - kLineWords))
def _(headers):
    # olo is a multiple of kLineWords, so 60 words is the largest distance to a unit base
    return [3 * 1024 + 900, 6000, 10 * 1024 + 930 - (3 * 1024 + 900) - 6000, 4100, 100]  # frames 1 and 3


def _check_owned_end(rem):
    def check(g):
        w = g.frame_words()
        span = w["ohi"] - w["b0"]
        assert np.any((w["units"][:-1] >= 2) & (span[:-1] % kUnitWords == rem))
    return check


def _owned_end_case(tag, rem):
    @_case(f"unit_owned_end_{tag}", "unit", check=_check_owned_end(rem))
    def _(headers):
        # frame 1 starts at 1 KiB + 10 and ends `rem` words past two whole units
        end = 1024 + 2 * 16 * kUnitWords + 16 * rem
        return [1034, end - 1034 - 20, 20 + 700, 2 * 16 * kUnitWords - 700, 300]


_owned_end_case("on_unit_boundary", 0)
_owned_end_case("one_granule_past_unit_boundary", kLineWords)


def _check_interior_end(g):
    w = g.frame_words()
    assert np.any((w["units"] >= 2) & ((w["ihi"] - w["b0"]) % kUnitWords == 0) & (w["ohi"] > w["ihi"]) &
                  (w["ihi"] > w["ilo"]))


@_case("unit_interior_edge_on_unit_boundary", "unit", check=_check_interior_end)
def _(headers):
    # frame 1's payload ends 5 bytes past a unit boundary: the unit before it is
    # all interior, the next one starts with the tail words
    a = 1024 + 16 * kUnitWords + 5
    return [1000, a - 1000, 3000, 100]


def _check_last_granule(g):
    w = g.frame_words()
    assert g.total % 16 == 1 and 16 * int(w["ohi"][-1]) >= g.total + 32 and w["units"][-1] >= 1


@_case("unit_last_granule_clipped", "unit", check=_check_last_granule)
def _(headers):
    return [3000, 500, 64 * 100 + 17 - 3500]


# ------------------------------ parametrised families ------------------------------
COUNT_EDGES = (255, 256, 257, 2047, 2048, 2049, 4097)
COUNT_LENS = (0, 1, 7, 125, 126, 300, 4096)


def frame_count_batch(n, headers):
    """n frames with lengths mixed over COUNT_LENS (every row and tile has its
    own offset); masked and unmasked frames for encode."""
    rng = np.random.default_rng(1000 + n)
    lens = rng.choice(COUNT_LENS, size=n).astype(np.int64)
    mask = rng.integers(0, 2, size=n) if headers else np.ones(n, dtype=np.int64)
    flags = (FIN_BINARY | (mask << 8)).astype(np.uint32)
    src, offs, keys = layout_source(f"count-{n}-{int(headers)}", lens)
    return src, offs, lens, flags, keys


PHASE_LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 4096 + 16 * 63 + 9)


def phase_batch(out_phase, headers, mixed_masks=False):
    """One batch per output phase: for every length class and source phase a
    pad frame that puts the next payload's first byte at `out_phase` (mod 16),
    then a payload of that class read from that source phase.  mixed_masks
    (encode): frames alternate between masked and unmasked."""
    lens, flags, phases = [], [], []
    cur = 0
    for ci, L in enumerate(PHASE_LENS):
        for ps in range(16):
            mask = (ci + ps) & 1 if (headers and mixed_masks) else 1
            hl = int(header_len(L, mask)) if headers else 0
            pad_hl = 2 + 4 * mask if headers else 0
            pad = (out_phase - hl - cur - pad_hl) % 16  # the pad's payload
            for length, phase in ((pad, 0), (L, ps)):
                lens.append(length)
                flags.append(FIN_BINARY | (mask << 8))
                phases.append(phase)
            cur += pad_hl + pad + hl + L
    lens = np.array(lens, dtype=np.int64)
    flags = np.array(flags, dtype=np.uint32)
    src, offs, keys = layout_source(f"phase-{out_phase}-{int(headers)}-{int(mixed_masks)}", lens, phases)
    return src, offs, lens, flags, keys


# ------------------------------ boundary-count parameters ------------------------------
def search_boundary_params(target, headers):
    """The first (shifter, X, small, delta) whose chunk 1 lists exactly `target`
    boundary words with at most kChunkFrames frames (used once to fill the
    table below; kept so a retune can regenerate it)."""
    for delta in (0, 5):
        for small in (32, 48, 38, 22):
            for s in range(6, 40):
                for x in range(8, 62):
                    regions, deltas = _boundary_regions(target, headers, (s, x, small, delta))
                    try:
                        lens, flags = frames_from_regions(regions, headers)
                    except ValueError:
                        continue
                    g0 = Geometry(np.zeros(len(lens)), lens, flags, headers)
                    g = Geometry((g0.p0 + delta) & 15, lens, flags, headers)
                    if g.chunk_nfr()[1] <= kChunkFrames and g.chunk_boundary_words(1) == target:
                        return s, x, small, delta
    return None
