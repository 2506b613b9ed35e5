"""The device helpers every large test and bench.py's "every byte verified" rest
on -- kmws_check_unmasked, kmws_fill_synthetic, kmws_fill_uniform_descs --
against the host: orc.synthetic, orc.splitmix64, orc.unmask_batch and numpy.

The checker is asserted `== 0` all over the suite; here it is asserted to COUNT:
on a small irregular batch (misaligned frames, empty frames, gaps; a span that
is no multiple of 16) every corruption returns exactly the number of bytes numpy
finds different from the oracle's image, and on a span of 2^32 + 2^27 bytes one
flipped byte returns 1 wherever it lies: in the second grid-stride pass, on both
sides of 2^31 and 2^32, and at the last byte.

Mutants of check_unmasked_kernel (each built from a scratch copy of
kmws_unmask.hip and run once against this file on an MI355X) and the tests
that failed; nothing else in the suite asserts a nonzero count, so nothing
else could:

  no grid-stride loop (a block checks its first 4 KiB only)
      -> test_reach_one_flip, all 8: second_pass, 2^31-1 .. 2^32+1, last, all
         (every probed position lies past the first 256 MiB: each returned 0)
  key phase dropped (key byte picked by p & 3 instead of (p - off) & 3)
      -> test_small_batch_counts, all 9, [clean] first (misaligned frames
         count as wrong), and test_two_calls_on_one_counter_add
  position cut to 32 bits (p & 0xFFFFFFFF before the load and the generator)
      -> test_reach_clean_and_sampled_against_the_oracle (the bytes past 2^32
         are compared with the wrong frame) and test_reach_one_flip, all 8
  bytes outside frames ignored (only covered bytes compared)
      -> test_small_batch_counts[gap_byte], [span_byte_0], [span_last_byte],
         [scattered_37], and test_two_calls_on_one_counter_add
"""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SEED = 0x5EED1234
ZERO_BYTE_KEY = 0x7100A5C3  # byte 2 is zero: a frame left masked differs in 3 bytes of every 4


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


# ------------------------------ the small batch ------------------------------
def small_batch():
    """The packed_wire, zero_len_runs and sparse_gaps layouts of
    tests/test_gpu_unmask.py back to back, cut down to under 1 MiB; 5 bytes of
    tail, so the span is no multiple of 16."""
    rng = np.random.default_rng(20240611)
    offs, lens = [], []
    pos = 0
    # packed_wire: payloads behind 6..14-byte headers (misaligned starts)
    for L in [0, 1, 7, 125, 126, 1000, 4096, 65535, 65536, 70001] + list(rng.choice([0, 1, 7, 125, 126, 1000, 4096],
                                                                                    size=30)):
        pos += (2 if L <= 125 else 4 if L <= 65535 else 10) + 4
        offs.append(pos)
        lens.append(int(L))
        pos += int(L)
    # zero_len_runs: empty frames at equal offsets, adjacent frames, no gaps
    for L in rng.choice([0, 0, 0, 1, 2, 3, 17, 300], size=600):
        offs.append(pos)
        lens.append(int(L))
        pos += int(L)
    # sparse_gaps: holes between frames
    for L, g in zip(rng.integers(1, 5000, size=24), rng.integers(1, 20000, size=24)):
        pos += int(g)
        offs.append(pos)
        lens.append(int(L))
        pos += int(L)
    span = pos + 5
    while span % 16 == 0 or span % 4096 == 0:
        span += 1
    assert span <= 1 << 20
    n = len(offs)
    keys = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    keys[::17] = 0
    d = np.zeros(n, dtype=orc.DESC_DTYPE)
    d["off"], d["len"], d["key"] = offs, lens, keys
    return d, span


@pytest.fixture(scope="module")
def small(T):
    """(descs, span, device descs, the oracle's unmasked image, the device's)."""
    from kuma_amd import kmws
    d, span = small_batch()
    masked_frame = int(np.flatnonzero(d["len"] == 70001)[0])
    d["key"][masked_frame] = ZERO_BYTE_KEY
    want = orc.synthetic(SEED, 0, span)
    orc.unmask_batch(want, d)
    base = T.zeros(span + 16 - span % 16, dtype=T.uint8, device="cuda")
    kmws.fill_synthetic(base, SEED, span)
    d_desc = T.from_numpy(d.view(np.int64).reshape(-1, 2).copy()).cuda()
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    kmws.unmask_batch(base, d_desc, ws, span)
    T.cuda.synchronize()
    assert ws.status() == 0
    got = base[:span].cpu().numpy()
    assert np.array_equal(got, want)
    return dict(d=d, span=span, d_desc=d_desc, want=want, masked_frame=masked_frame)


def key_bytes(key, length, rot=0):
    kb = np.array([(int(key) >> (8 * ((i + rot) & 3))) & 0xFF for i in range(4)], dtype=np.uint8)
    return np.tile(kb, length // 4 + 1)[:length]


def corrupt(name, s):
    """(the corrupted image, the count the corruption makes by construction)."""
    d, span, img = s["d"], s["span"], s["want"].copy()
    covered = np.zeros(span, dtype=bool)
    for o, L in zip(d["off"], d["len"]):
        covered[int(o):int(o) + int(L)] = True
    big = int(np.flatnonzero(d["len"] == 65535)[0])
    o, L = int(d["off"][big]), int(d["len"][big])
    if name == "clean":
        return img, 0
    if name == "payload_byte_0":
        assert o % 16 != 0
        img[o] ^= 0xFF
        return img, 1
    if name == "payload_last_byte":
        img[o + L - 1] ^= 0x01
        return img, 1
    if name == "gap_byte":
        last = len(d) - 1  # the sparse_gaps section: the byte before the last frame is a gap
        p = int(d["off"][last]) - 1
        assert not covered[p]
        img[p] ^= 0x80
        return img, 1
    if name == "span_byte_0":
        assert not covered[0]
        img[0] ^= 0xFF
        return img, 1
    if name == "span_last_byte":
        assert not covered[span - 1] and (span - 1) % 16 != 15
        img[span - 1] ^= 0xFF
        return img, 1
    f = s["masked_frame"]
    o, L, key = int(d["off"][f]), int(d["len"][f]), int(d["key"][f])
    assert o % 4 != 0  # the key phase is the payload's, not the address's
    if name == "frame_left_masked":
        kb = key_bytes(key, L)
        img[o:o + L] ^= kb
        assert 0 in [(key >> (8 * i)) & 0xFF for i in range(4)]
        return img, int(np.count_nonzero(kb))
    if name == "key_rotated":
        diff = key_bytes(key, L) ^ key_bytes(key, L, rot=1)  # unmasked with the rotated key instead
        img[o:o + L] ^= diff
        return img, int(np.count_nonzero(diff))
    if name == "scattered_37":
        rng = np.random.default_rng(37)
        p = rng.choice(span, size=37, replace=False)
        img[p] ^= rng.integers(1, 256, size=37, dtype=np.uint8)
        return img, 37
    raise ValueError(name)


CORRUPTIONS = ["clean", "payload_byte_0", "payload_last_byte", "gap_byte", "span_byte_0", "span_last_byte",
               "frame_left_masked", "key_rotated", "scattered_37"]


@pytest.mark.parametrize("name", CORRUPTIONS)
def test_small_batch_counts(T, small, name):
    """The checker returns exactly the number of bytes that differ from the
    oracle's unmasked image (numpy's count == the count by construction)."""
    from kuma_amd import kmws
    img, by_construction = corrupt(name, small)
    by_numpy = int(np.count_nonzero(img != small["want"]))
    assert by_numpy == by_construction
    span = small["span"]
    dev = T.from_numpy(np.concatenate([img, np.zeros(16 - span % 16, np.uint8)])).cuda()
    got = kmws.check_unmasked(dev, SEED, small["d_desc"], span)
    print(name, "checker", got, "numpy", by_numpy)
    assert got == by_numpy


def test_two_calls_on_one_counter_add(T, small):
    """include/kmws_bench.h: *mismatches is accumulated, not overwritten."""
    from kuma_amd import kmws
    span = small["span"]
    cnt = T.full((1,), 1000, dtype=T.int64, device="cuda")
    total = 1000
    for name in ("scattered_37", "clean", "frame_left_masked"):
        img, k = corrupt(name, small)
        dev = T.from_numpy(np.concatenate([img, np.zeros(16 - span % 16, np.uint8)])).cuda()
        assert kmws.lib().kmws_check_unmasked(dev.data_ptr(), span, SEED, small["d_desc"].data_ptr(),
                                              len(small["d"]), cnt.data_ptr(), kmws._stream_handle()) == 0
        total += k
        assert int(cnt.item()) == total, name


# ------------------------------ reach: 2^32 + 2^27 bytes ------------------------------
BIG_SPAN = (1 << 32) + (1 << 27)
FRAME = 65536
BIG_SEED, BIG_KEY_SEED = 424242, 99
REACH = {
    "second_pass": (256 << 20) + 4096 * 3 + 17,  # block 65536 + 3: the checker's second grid-stride pass
    "2^31-1": (1 << 31) - 1, "2^31": 1 << 31,
    "2^32-1": (1 << 32) - 1, "2^32": 1 << 32, "2^32+1": (1 << 32) + 1,
    "last": BIG_SPAN - 1,
}


@pytest.fixture(scope="module")
def big(T):
    """The span unmasked once by kmws_unmask_batch; freed when the module is done."""
    from kuma_amd import kmws
    n = BIG_SPAN // FRAME
    base = T.empty(BIG_SPAN, dtype=T.uint8, device="cuda")
    descs = T.empty((n, 2), dtype=T.int64, device="cuda")
    kmws.fill_synthetic(base, BIG_SEED)
    kmws.fill_uniform_descs(descs, FRAME, FRAME, BIG_KEY_SEED)
    ws = kmws.Workspace(kmws.unmask_workspace_size(BIG_SPAN))
    kmws.unmask_batch(base, descs, ws, BIG_SPAN)
    T.cuda.synchronize()
    assert ws.status() == 0
    del ws
    yield base, descs
    del base, descs
    T.cuda.empty_cache()


def test_reach_clean_and_sampled_against_the_oracle(T, big):
    """0 on the correct span, and the bytes around every probed position equal
    the oracle's (the flips below start from a right image)."""
    from kuma_amd import kmws
    base, descs = big
    assert kmws.check_unmasked(base, BIG_SEED, descs) == 0
    for p in REACH.values():
        i = p // FRAME
        want = orc.synthetic(BIG_SEED, i * FRAME, FRAME)
        d = np.zeros(1, dtype=orc.DESC_DTYPE)
        d["off"], d["len"], d["key"] = 0, FRAME, orc.splitmix64(BIG_KEY_SEED + i) & 0xFFFFFFFF
        orc.unmask_batch(want, d)
        assert np.array_equal(base[i * FRAME:(i + 1) * FRAME].cpu().numpy(), want), p


@pytest.mark.parametrize("where", list(REACH) + ["all"])
def test_reach_one_flip(T, big, where):
    """One byte ^ 0xFF at the position: exactly 1; all positions: their number."""
    from kuma_amd import kmws
    base, descs = big
    pos = list(REACH.values()) if where == "all" else [REACH[where]]
    assert all(0 <= p < BIG_SPAN for p in pos) and len(set(pos)) == len(pos)
    idx = T.tensor(pos, dtype=T.int64, device="cuda")
    base[idx] ^= 0xFF
    try:
        got = kmws.check_unmasked(base, BIG_SEED, descs)
    finally:
        base[idx] ^= 0xFF
    print(where, "checker", got)
    assert got == len(pos)


# ------------------------------ the generators ------------------------------
def test_fill_synthetic_windows_past_4_gib(T):
    """kmws_fill_synthetic == orc.synthetic on 64 KiB windows at 0, around 2^31,
    around 2^32 and at the end of a 2^32 + 2^27 - 3 byte fill (13 bytes through
    the 1-15 byte tail path), and nothing written past the fill."""
    from kuma_amd import kmws
    nbytes = BIG_SPAN - 3
    assert nbytes % 16 == 13
    W = 65536
    base = T.empty(BIG_SPAN, dtype=T.uint8, device="cuda")
    base[BIG_SPAN - 16:] = 0xEE
    kmws.fill_synthetic(base, 777, nbytes)
    T.cuda.synchronize()
    for a in (0, (1 << 31) - W // 2, (1 << 32) - W // 2, nbytes - W):
        assert np.array_equal(base[a:a + W].cpu().numpy(), orc.synthetic(777, a, W)), a
    assert base[nbytes:].cpu().tolist() == [0xEE] * 3
    del base
    T.cuda.empty_cache()


def host_keys(seed, n):
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)


@pytest.mark.parametrize("stride,length", [(65536, 65536), (65521 * 3, 70001)], ids=["64k", "not_a_power_of_two"])
def test_fill_uniform_descs_past_4_gib(T, stride, length):
    """All of n = 70,000 descriptors == {i * stride, len, low 32 bits of
    splitmix64(seed + i)}; i * stride passes 2^32 in both."""
    from kuma_amd import kmws
    n, seed = 70000, 0xABCDEF0123
    descs = T.full((n + 1, 2), -1, dtype=T.int64, device="cuda")
    kmws.fill_uniform_descs(descs[:n], stride, length, seed)
    T.cuda.synchronize()
    h = descs.cpu().numpy()
    got = h[:n].copy().view(orc.DESC_DTYPE).reshape(-1)
    want_off = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    assert int(want_off[-1]) > 1 << 32
    assert np.array_equal(got["off"], want_off)
    assert np.all(got["len"] == length)
    keys = host_keys(seed, n)
    for i in (0, 1, 65535, 65536, n - 1):
        assert int(keys[i]) == orc.splitmix64(seed + i) & 0xFFFFFFFF
    assert np.array_equal(got["key"], keys)
    assert h[n].tolist() == [-1, -1]  # nothing past n
