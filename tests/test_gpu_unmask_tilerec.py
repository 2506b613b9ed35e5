"""GPU parity of the unmask plan's per-tile records (kmws::TileRec: frame
index, "one frame covers this tile" flag, rotated key) and of the block ->
tile mapping computed without division, byte for byte against
oracle.unmask_batch, gaps and headers included.

A tile is 16 KiB.  The cases sit where a record can be wrong: frames that
start or end on, one byte after or one byte before a tile edge, a frame over
several whole tiles, a key-0 covered tile, empty frames, the partial last
tile; spans whose tile count leaves a remainder in every mapping; a workspace
planned twice; and the fused parse + plan kernel."""
import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

T = 16384  # the product tile
NT, TEMPORAL = 1 << 29, 1 << 30
KINDS_X_STORES = [k | s for k in range(6) for s in (NT, TEMPORAL)]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


def make_descs(offs, lens, keys):
    d = np.zeros(len(offs), dtype=orc.DESC_DTYPE)
    d["off"], d["len"], d["key"] = offs, lens, keys
    return d


def to_dev(torch, buf, descs):
    d_buf = torch.from_numpy(np.concatenate([buf, np.zeros((-len(buf)) % 16, np.uint8)])).cuda()
    d_desc = torch.from_numpy(descs.view(np.int64).reshape(-1, 2).copy()).cuda()
    return d_buf, d_desc


def oracle_of(buf, descs):
    want = buf.copy()
    orc.unmask_batch(want, descs)
    return want


def records(ws, ntiles):
    """The workspace's tile records as (frame word, key word) uint32 columns, sentinel included."""
    raw = ws.tensor[16:16 + 8 * (ntiles + 1)].cpu().numpy().view(np.uint32).reshape(-1, 2)
    return raw[:, 0], raw[:, 1]


def boundary_batch():
    span = 9 * T + 40
    frames = [
        (0, T - 1, 0x11223344),            # starts on a tile start, ends one byte before the tile end
        (T - 1, 0, 0xDEADBEEF),            # two empty frames between payloads
        (T - 1, 0, 0x01020304),
        (T + 1, T - 1, 0xA1B2C3D4),        # starts one byte after a tile start, ends on the tile end
        (2 * T, 3 * T, 0x0badf00d),        # covers three whole tiles
        (5 * T + 5001, T - 5001, 0x55667788),  # starts mid-tile (odd phase), ends on the tile end
        (6 * T, T, 0),                     # key 0 over a whole tile
        (7 * T + 3, T - 4, 0x99aabbcc),    # one byte short at the end, three past the start
        (8 * T + 100, T - 100 + 33, 0x31415926),  # ends in the partial last tile
    ]
    offs, lens, keys = zip(*frames)
    assert offs[-1] + lens[-1] <= span
    return span, make_descs(offs, lens, keys)


@pytest.mark.parametrize("schedule", [None, 1 | NT, 3 | TEMPORAL, 0 | NT])
def test_tile_boundary_cases(torch_dev, schedule):
    from kuma_amd import kmws
    span, descs = boundary_batch()
    buf = np.random.default_rng(1).integers(0, 256, size=span, dtype=np.uint8)
    want = oracle_of(buf, descs)
    d_buf, d_desc = to_dev(torch_dev, buf, descs)
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    kmws.unmask_batch(d_buf, d_desc, ws, span, schedule=schedule)
    torch_dev.cuda.synchronize()
    assert ws.status() == 0
    assert np.array_equal(d_buf.cpu().numpy()[:span], want)
    # the records themselves: tiles 2, 3, 4 (frame 4) and 6 (frame 6, key 0) are covered, nothing else
    fw, kw = records(ws, 10)
    covered = (fw >> 31).astype(bool)
    assert covered.tolist() == [False, False, True, True, True, False, True, False, False, False, False]
    assert (fw & 0x7FFFFFFF).tolist() == [0, 2, 4, 4, 4, 4, 6, 6, 7, 8, 8]
    assert kw[2:5].tolist() == [0x0badf00d] * 3 and kw[6] == 0


@pytest.mark.parametrize("off,length", [(0, T + 16), (0, T), (3, T + 13), (1, 2)])
def test_single_frame_one_tile_and_a_word(torch_dev, off, length):
    from kuma_amd import kmws
    span = T + 16
    descs = make_descs([off], [length], [0xC0FFEE11])
    buf = np.random.default_rng(2).integers(0, 256, size=span, dtype=np.uint8)
    want = oracle_of(buf, descs)
    d_buf, d_desc = to_dev(torch_dev, buf, descs)
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    kmws.unmask_batch(d_buf, d_desc, ws, span)
    torch_dev.cuda.synchronize()
    assert ws.status() == 0 and np.array_equal(d_buf.cpu().numpy()[:span], want)
    fw, _ = records(ws, 2)
    assert bool(fw[0] >> 31) == (off == 0 and length >= T) and not fw[1] >> 31 and not fw[2] >> 31


@pytest.fixture(scope="module", params=[131, 67], ids=["131_tiles", "67_tiles"])
def remainder_batch(request, torch_dev):
    """Uniform 65,531-byte frames at stride 65,536 over `tiles` tiles + 40 B: the
    input on the host, its descriptors on the device and the oracle's result, made once."""
    tiles = request.param
    span = tiles * T + 40
    n = span // 65536
    offs = np.arange(n, dtype=np.uint64) * 65536
    keys = np.random.default_rng(tiles).integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    descs = make_descs(offs, np.full(n, 65531), keys)
    buf = np.random.default_rng(tiles + 1).integers(0, 256, size=span, dtype=np.uint8)
    want = oracle_of(buf, descs)
    buf.setflags(write=False)
    want.setflags(write=False)
    return span, buf, descs, want


@pytest.mark.parametrize("schedule", [None] + KINDS_X_STORES)
def test_every_mapping_with_a_remainder(torch_dev, remainder_batch, schedule):
    """131 tiles: whole rounds plus leftover tiles in every kind; 67: the run
    kinds fall back to in order, split 8 has q = 8 with 3 tiles left.  One plan,
    three applies (odd): a skipped or doubled tile, or a record consumed or
    left stale by an apply, breaks parity."""
    from kuma_amd import kmws
    span, buf, descs, want = remainder_batch
    d_buf, d_desc = to_dev(torch_dev, np.array(buf), descs)
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    kmws.unmask_plan(d_desc, ws, span)
    for _ in range(3):
        kmws.unmask_apply(d_buf, d_desc, ws, span, schedule=schedule)
    torch_dev.cuda.synchronize()
    assert ws.status() == 0
    assert np.array_equal(d_buf.cpu().numpy()[:span], want)


def test_replan_on_the_same_workspace(torch_dev):
    """Large frames (most tiles covered), then 3,000-byte frames over the same
    span through the same workspace: parity, and no covered record survives."""
    from kuma_amd import kmws
    tiles = 131
    span = tiles * T + 40
    rng = np.random.default_rng(7)
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    n1 = span // 65536
    big = make_descs(np.arange(n1, dtype=np.uint64) * 65536, np.full(n1, 65531),
                     rng.integers(0, 2**32, size=n1, dtype=np.uint64).astype(np.uint32))
    n2 = span // 4096
    small = make_descs(np.arange(n2, dtype=np.uint64) * 4096 + 7, np.full(n2, 3000),
                       rng.integers(0, 2**32, size=n2, dtype=np.uint64).astype(np.uint32))
    seen_covered = []
    for descs in (big, small):
        buf = rng.integers(0, 256, size=span, dtype=np.uint8)
        want = oracle_of(buf, descs)
        d_buf, d_desc = to_dev(torch_dev, buf, descs)
        kmws.unmask_batch(d_buf, d_desc, ws, span)
        torch_dev.cuda.synchronize()
        assert ws.status() == 0
        assert np.array_equal(d_buf.cpu().numpy()[:span], want)
        fw, _ = records(ws, tiles + 1)
        seen_covered.append(int((fw >> 31).sum()))
    assert seen_covered[0] == 3 * n1 and seen_covered[1] == 0  # 3 of a frame's 4 tiles hold payload only


def test_fused_unpack_unmask_writes_the_same_records(torch_dev):
    """kmws_unpack_unmask on a small mixed wire of masked frames: the wire equals
    the oracle's unmask, and unpack_plan_kernel marks the same tiles covered, with
    the same frame and key, as tile_map_kernel does."""
    torch = torch_dev
    from kuma_amd import kmws
    rng = np.random.default_rng(11)
    lens = [5, 70000, 3 * T + 7, 0, 200, 40000, 125, 126, 65536, 2 * T]
    wire, hdr_off, offs, keys = b"", [], [], []
    for L in lens:
        key = bytes(rng.integers(0, 256, size=4, dtype=np.uint8))
        h = orc.encode_header(orc.Hdr(opcode=2, mask=1, maskey=key, length=L))
        hdr_off.append(len(wire))
        offs.append(len(wire) + len(h))
        keys.append(int.from_bytes(key, "little"))
        wire += h + bytes(rng.integers(0, 256, size=L, dtype=np.uint8))
    W = len(wire)
    buf = np.frombuffer(wire, dtype=np.uint8).copy()
    descs = make_descs(offs, lens, keys)
    want = oracle_of(buf, descs)
    n = len(lens)
    d_buf, d_desc = to_dev(torch, buf, descs)
    d_hdr = torch.from_numpy(np.array(hdr_off, dtype=np.uint64).view(np.int64)).cuda()
    out_desc = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    out_err = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
    ws = kmws.Workspace(kmws.unmask_workspace_size(W))
    kmws.unpack_unmask(d_buf, d_hdr, kmws.SERVER, out_desc, None, out_err, ws, wire_len=W)
    torch.cuda.synchronize()
    assert ws.status() == 0 and int(out_err.max()) == 0
    assert torch.equal(out_desc, d_desc)
    assert np.array_equal(d_buf.cpu().numpy()[:W], want)
    ntiles = (W + T - 1) // T
    fused = records(ws, ntiles)
    ws2 = kmws.Workspace(kmws.unmask_workspace_size(W))
    kmws.unmask_plan(d_desc, ws2, W)
    torch.cuda.synchronize()
    planned = records(ws2, ntiles)
    # the two plans cut regions at header and at payload offsets, so a tile that starts
    # inside a header may name either neighbour; a covered tile has one answer
    cov = (planned[0] >> 31).astype(bool)
    assert np.array_equal((fused[0] >> 31).astype(bool), cov) and int(cov.sum()) >= 8
    assert np.array_equal(fused[0][cov], planned[0][cov]) and np.array_equal(fused[1], planned[1])
