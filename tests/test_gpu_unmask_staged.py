"""GPU parity of the capped apply launches (unmask_split_kernel<V, TWO = true>)
tile kind by tile kind: covered tiles (the path whose loads are staged by
kUnmaskDepth), two-frame tiles, the LDS path inside a capped launch and the
tail kernel, in one small batch; a bad plan; and a batch of four times the
largest residency of the (blocks, depth) grid, so that every block slot of a
CU turns over many times.  Byte for byte against the oracle, gaps included,
under the default schedule and all 6 placement kinds x both store bits."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

T = 16384  # the apply's tile
SCHEDULES = [None] + [k | s for k in range(6) for s in (1 << 29, 1 << 30)]  # kind x NT / temporal

# (off, len, key): 9 tiles + 100 bytes, 8 frames, mean region >= one tile (capped).
# off & 3 takes every residue, twice each, no two neighbours alike.
FRAMES = [
    (5, 3 * T + 7 - 5, 0x9C3A51E7),             # from byte 5 of tile 0 to 7 bytes into tile 3
    (3 * T + 10, 100, 0x01020304),              # three short frames inside tile 3 ...
    (3 * T + 115, 1, 0xA0B0C0D0),
    (3 * T + 121, 4000, 0x7F00FF80),            # ... with the first frame's end: the LDS path
    (4 * T, 0, 0x11223344),                     # zero length at a tile start
    (4 * T + 6, 20003, 0),                      # key 0, across tiles 4 and 5
    (4 * T + 6 + 20003 + 14, 0, 0xDEADBEEF),    # after a 14-byte gap, to the end of tile 7 exactly (len below)
    (8 * T + 4, T + 40, 0x5EED1234),            # ends in the partial last tile: the tail kernel
]
SPAN = 9 * T + 100
WANT_KINDS = ["two", "covered", "covered", "general", "two", "two", "covered", "covered", "two", "tail"]


def _descs():
    d = np.zeros(len(FRAMES), dtype=orc.DESC_DTYPE)
    for i, (off, ln, key) in enumerate(FRAMES):
        d["off"][i], d["len"][i], d["key"][i] = off, ln, key
    d["len"][6] = 8 * T - int(d["off"][6])
    return d


def _tile_kinds(d, span):
    """What the plan and the apply make of each tile, recomputed from the
    descriptors: frame f owns the tile starts in [off_f, off_{f+1}) (from 0 for
    the first, to the span for the last)."""
    offs = d["off"].astype(np.int64)
    ends = offs + d["len"].astype(np.int64)
    n = len(d)

    def owner(x):
        return max(int(np.searchsorted(offs, x, side="right")) - 1, 0)

    kinds = []
    for t in range((span + T - 1) // T):
        lo, hi = t * T, (t + 1) * T
        if hi > span:
            kinds.append("tail")
            continue
        f = owner(lo)
        flast = owner(hi) if hi < span else n - 1
        if offs[f] <= lo and ends[f] >= hi:
            kinds.append("covered")
        elif flast <= f + 1:
            kinds.append("two")
        else:
            kinds.append("general")
    return kinds


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


@pytest.fixture(scope="module")
def mixed():
    """(buffer, descriptors, oracle result): computed once, never written."""
    d = _descs()
    buf = np.random.default_rng(20250).integers(0, 256, size=SPAN, dtype=np.uint8)
    want = buf.copy()
    orc.unmask_batch(want, d)
    for a in (buf, want):
        a.setflags(write=False)
    return buf, d, want


def _run(torch, buf, d, span, schedule):
    from kuma_amd import kmws
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros((-len(buf)) % 16, np.uint8)])).cuda()
    d_desc = torch.from_numpy(d.view(np.int64).reshape(-1, 2).copy()).cuda()
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    kmws.unmask_batch(d_buf, d_desc, ws, span, schedule=schedule)
    torch.cuda.synchronize()
    return d_buf.cpu().numpy()[:len(buf)], ws.status()


def test_mixed_batch_layout_is_what_its_name_claims(mixed):
    _, d, _ = mixed
    offs, lens = d["off"].astype(np.int64), d["len"].astype(np.int64)
    assert SPAN // len(d) >= T  # the capped launches
    assert np.all(offs[1:] >= offs[:-1] + lens[:-1]) and offs[-1] + lens[-1] <= SPAN
    res = (offs & 3).tolist()
    assert sorted(res) == [0, 0, 1, 1, 2, 2, 3, 3] and all(a != b for a, b in zip(res, res[1:]))
    assert offs[0] == 5 and offs[0] + lens[0] == 3 * T + 7
    assert offs[6] - (offs[5] + lens[5]) == 14 and (offs[6] + lens[6]) % T == 0
    assert lens[4] == 0 and offs[4] % T == 0
    assert d["key"][5] == 0 and offs[5] // T + 1 == (offs[5] + lens[5] - 1) // T
    assert lens[1:4].tolist() == [100, 1, 4000] and offs[1] // T == (offs[3] + lens[3] - 1) // T == 3
    assert (offs[7] + lens[7]) > 9 * T
    assert _tile_kinds(d, SPAN) == WANT_KINDS


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_mixed_tile_kinds_parity(torch_dev, mixed, schedule):
    buf, d, want = mixed
    assert _tile_kinds(d, SPAN) == WANT_KINDS
    got, st = _run(torch_dev, buf, d, SPAN, schedule)
    assert st == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_bad_plan_stores_nothing(torch_dev, mixed, schedule):
    buf, d, _ = mixed
    bad = d.copy()
    bad[[2, 6]] = bad[[6, 2]]  # two descriptors swapped: offsets out of order
    got, st = _run(torch_dev, buf, bad, SPAN, schedule)
    assert st & 1
    assert np.array_equal(got, buf)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_covered_tiles_turnover(torch_dev, schedule):
    """8,192 covered tiles (128 MiB of 64 KiB frames): four times the 2,048
    blocks the largest residency of the grid (8 per CU) keeps in flight.
    Applied three times (odd), every byte checked on the device."""
    torch = torch_dev
    from kuma_amd import kmws
    L, span, seed = 65536, 8192 * T, 4321
    base = torch.empty(span, dtype=torch.uint8, device="cuda")
    descs = torch.empty((span // L, 2), dtype=torch.int64, device="cuda")
    kmws.fill_synthetic(base, seed)
    kmws.fill_uniform_descs(descs, L, L, 77)
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    for _ in range(3):
        kmws.unmask_batch(base, descs, ws, span, schedule=schedule)
    torch.cuda.synchronize()
    assert ws.status() == 0
    assert kmws.check_unmasked(base, seed, descs) == 0
