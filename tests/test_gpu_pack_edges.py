"""Structure-edge parity of the encode / gather copy kernels (kmws_pack.hip)
against the oracle, byte for byte: the deterministic cases of
tests/pack_edge_cases.py (whose properties tests/test_pack_edge_cases.py
proves on the CPU) through kmws_encode_batch, kmws_gather_unmask and
kmws_unpack_gather, each in the chunk form and in the unit form.

The form is chosen through dst_cap alone (cap // n < 16384: chunks) and every
run asserts the side it is on, a clean workspace status, the offsets, the
total, dst[:total] and that EVERY byte of dst[total:] still holds the fill.

References: encode = the oracle's encode_batch; gather = the oracle's
unmask_batch on a copy of the source, its payload slices back to back; the
fused unpack-gather reads the oracle's masked wire of the gather variant's
payloads and must give the source slices, the oracle decoder's payloads and
what kmws_unpack_headers + kmws_gather_unmask give (payload phases in that
wire follow from the header sizes, so no phase property is claimed for it).

What each case pins in kmws_pack.hip, and the one-condition mutants of a
scratch copy of the source (never committed, all in bounds) that the named
tests caught on an MI355X when this file was written:

  chunk_nfr_64_65            the dense hand-off `nfr > kChunkFrames` and the count
                             in WsHead::pad[0].  `>=`: only this case fails (the
                             dense kernel is exact, the count is not).
  chunk_boundary_words_64..81  s_val slots 0..63 against the 16 scratch slots.
                             `pos < 64` -> `<= 64`: _81 fails (slot 64 then holds
                             word 80; with 65 or 80 words it still holds word 64,
                             so the flip is harmless there) and chunk_nfr_64_65;
                             `g0 >= 64` -> `> 64`: _65, _80, _81 fail.
  chunk_lane63_extra_load    word 255 interior: without the `lane != 63` term of
                             `nb` it fails, with every chunk-form run of a long
                             shifted payload (count edges, phase pairs, ...).
  chunk_payload_end_edge_*   a payload's last interior / first boundary word at
  chunk_total_*              a chunk edge; trel, store_word_bytes, a + 16 <= total.
  empty_*                    cmap and the frame table over runs of empty regions,
                             a whole empty scan tile, f1 = n - 1, nch = 0.
  unit_region_end_granule_*  ohi / ihi at a granule edge.  unit_finish's
  unit_interior_edge_...     `k == x.last` -> `x.last + 1`: every unit-form run
                             with a shifted interior fails.
  unit_zero_granule_frames   units == 0 slots; with unit_olo_minus_b0_*,
  unit_owned_end_*           unit_owned_end_* the cases that fail when make_rec's
                             rel() loses its upper clamp.
  unit_third_region_head     the `third` bits of row_prologue: `F.r1 < ah + 16`
  unit_third_region_tail_0..3  -> `< ah` fails _head; `N.r1 < a + 16` -> `< a`
                             fails _tail_0..3 (and _head, zero_granule).
  unit_last_granule_clipped  owned words past the total are never stored.

olo - b0 is a multiple of kLineWords (4), so its largest value is 60 words,
not 63: unit_olo_minus_b0_60 is the far end."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pack_edge_cases as pec  # noqa: E402
from oracle import oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0xEE
FORMS = ("chunks", "units")


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


def to_dev(T, a):
    pad = (-len(a)) % 16
    return T.from_numpy(np.concatenate([a, np.zeros(pad + 16, a.dtype)])).cuda()


def cap_for(form, n, total):
    """dst_cap that selects `form` for n frames, with room past the total on both sides of the rule."""
    cap = total + 5000 if form == "chunks" else max(total, pec.kChunkFormBelow * n) + 777
    assert (cap // n < pec.kChunkFormBelow) == (form == "chunks"), (form, n, cap)
    assert cap <= 70 << 20
    return cap


def dense_count(T, ws):
    """WsHead::pad[0]: the chunks chunk_copy_kernel handed to chunk_dense_kernel."""
    return int(ws.tensor[4:8].view(T.int32)[0])


def first_true(mask):
    idx = mask.nonzero()
    return int(idx[0]) if idx.numel() else None


class Batch:
    """One case on the device: inputs uploaded once, references computed once."""

    def __init__(self, T, batch, headers):
        from kuma_amd import kmws
        self.T, self.headers = T, headers
        src, offs, lens, flags, keys = batch
        self.n = len(lens)
        self.geom = pec.Geometry(offs, lens, flags, headers)
        self.d_src = to_dev(T, src)
        if headers:
            self.descs = kmws.make_descs(offs.astype(np.int64), lens, keys.astype(np.int64))
            self.flags = T.from_numpy(flags.astype(np.int16)).cuda()
            want, want_off = orc.encode_batch(src, offs, lens, flags, keys)
            self.want_off = want_off.astype(np.int64)
        else:
            # gather: the oracle unmasks the source in place; the slices back to back
            d = np.zeros(self.n, dtype=orc.DESC_DTYPE)
            d["off"], d["len"], d["key"] = offs, lens, keys
            base = src.copy()
            orc.unmask_batch(base, d)
            plain = [src[int(o):int(o) + int(L)] for o, L in zip(offs, lens)]
            want = np.concatenate([base[int(o):int(o) + int(L)] for o, L in zip(offs, lens)] + [np.zeros(0, np.uint8)])
            self.descs = kmws.make_descs(offs.astype(np.int64), lens, keys.astype(np.int64))
            self.want_off = self.geom.r0
            # the fused form's input: these payloads as a masked wire; its output: the plain slices
            wflags = np.full(self.n, pec.FIN_BINARY | pec.MASK_BIT, dtype=np.uint32)
            self.wire, wire_off = orc.encode_batch(src, offs, lens, wflags, keys)
            self.want_plain = np.concatenate(plain + [np.zeros(0, np.uint8)])
            rets, frames = orc.decode_chunks(bytes(self.wire), orc.SERVER, 0)
            assert len(frames) == self.n and b"".join(f.payload for f in frames) == bytes(self.want_plain)
            self.d_wire = to_dev(T, self.wire)
            self.d_hdr = T.from_numpy(wire_off.astype(np.int64)).cuda()
        self.total = len(want)
        assert self.total == self.geom.total
        self.d_want = T.from_numpy(np.ascontiguousarray(want)).cuda()
        self.d_want_off = T.from_numpy(np.concatenate([self.want_off, [self.total]]).astype(np.int64)).cuda()
        if not headers:
            self.d_plain = T.from_numpy(np.ascontiguousarray(self.want_plain)).cuda()

    def entries(self):
        return ("encode",) if self.headers else ("gather", "unpack_gather")

    def check(self, what, dst, off, ws, want, form):
        T = self.T
        T.cuda.synchronize()
        tag = (what, form, self.n, self.total)
        assert ws.status() == 0, tag
        assert T.equal(off, self.d_want_off), tag  # off[:n] and off[n] == total
        assert int(off[self.n]) == self.total, tag
        assert T.equal(dst[:self.total], want), tag + ("first wrong byte", first_true(dst[:self.total] != want))
        # nothing written past the total, anywhere
        assert bool((dst[self.total:] == FILL).all()), tag + ("first byte past the total", first_true(dst[self.total:] != FILL))
        if form == "chunks":
            assert dense_count(T, ws) == self.geom.dense_chunks(), tag

    def run(self, what, form, ws=None):
        """One call of entry `what` in `form`; returns the workspace (reusable)."""
        from kuma_amd import kmws
        T, n = self.T, self.n
        cap = cap_for(form, n, self.total)
        dst = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
        off = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
        ws = ws or kmws.Workspace(kmws.copy_workspace_size(n, cap))
        if what == "encode":
            kmws.encode_batch(self.d_src, self.descs, self.flags, dst, off, ws)
            self.check(what, dst, off, ws, self.d_want, form)
        elif what == "gather":
            kmws.gather_unmask(self.d_src, self.descs, dst, off, ws)
            self.check(what, dst, off, ws, self.d_want, form)
        else:
            W = len(self.wire)
            fd, ff, fe = (T.zeros((n, 2), dtype=T.int64, device="cuda"), T.zeros(n, dtype=T.int16, device="cuda"),
                          T.full((n,), 99, dtype=T.uint8, device="cuda"))
            kmws.unpack_gather(self.d_wire, self.d_hdr, kmws.SERVER, fd, ff, fe, dst, off, ws, wire_len=W)
            self.check(what, dst, off, ws, self.d_plain, form)  # the source slices = the oracle decoder's payloads
            assert int(fe.max()) == 0
            # the two-step form on the same wire, the same capacity
            od, of, oe = (T.zeros((n, 2), dtype=T.int64, device="cuda"), T.zeros(n, dtype=T.int16, device="cuda"),
                          T.full((n,), 99, dtype=T.uint8, device="cuda"))
            kmws.unpack_headers(self.d_wire, self.d_hdr, kmws.SERVER, od, of, oe, kmws.Workspace(16), wire_len=W)
            dst2 = T.full((cap,), FILL, dtype=T.uint8, device="cuda")
            off2 = T.full((n + 1,), -1, dtype=T.int64, device="cuda")
            ws2 = kmws.Workspace(kmws.copy_workspace_size(n, cap))
            kmws.gather_unmask(self.d_wire, od, dst2, off2, ws2)
            self.check("unpack+gather", dst2, off2, ws2, self.d_plain, form)
            assert T.equal(fd, od) and T.equal(ff, of) and T.equal(fe, oe)
            assert T.equal(dst, dst2) and T.equal(off, off2)
        return ws


def run_all(T, batch, headers, repeat=1):
    """Every applicable entry of the batch's template in both forms."""
    b = Batch(T, batch, headers)
    for what in b.entries():
        for form in FORMS:
            ws = None
            for _ in range(repeat):
                ws = b.run(what, form, ws)
    return b


def run_case(T, name):
    case = pec.CASES[name]
    for headers in case.variants():
        run_all(T, case.build(headers), headers)


@pytest.mark.parametrize("n", pec.COUNT_EDGES)
def test_copy_scan_frame_count_edges(T, n):
    """Row (256) and tile (2048) edges of the copy entries' scans: reduce +
    scan_tiles + prologue / chunk_map (unit form; the fused gather's chunk front,
    chunk_map_kernel with blockIdx.x >= 8 from n = 2049) and the one-pass
    chunk_scan_kernel.  Twice on one workspace: the tile states and the dense
    count are re-zeroed per call."""
    for headers in (True, False):
        run_all(T, pec.frame_count_batch(n, headers), headers, repeat=2)


@pytest.mark.parametrize("out_phase", range(16))
def test_copy_every_phase_pair(T, out_phase):
    """All 16 source phases x this output phase x 17 length classes in one
    batch; encode all masked and alternating masked / unmasked; keys include 0."""
    run_all(T, pec.phase_batch(out_phase, True), True)
    run_all(T, pec.phase_batch(out_phase, True, mixed_masks=True), True)
    run_all(T, pec.phase_batch(out_phase, False), False)


@pytest.mark.parametrize("name", [k for k, c in pec.CASES.items() if c.group == "chunk"])
def test_chunk_form_thresholds(T, name):
    """The chunk form's named thresholds.  Batch.check reads the dense-chunk
    count back from the workspace head and compares it with the model's count
    of chunks meeting more than 64 frames: the nfr case ran the path it names."""
    run_case(T, name)
    if name == "chunk_nfr_64_65":
        assert pec.CASES[name].geometry(True).dense_chunks() == 2


@pytest.mark.parametrize("name", [k for k, c in pec.CASES.items() if c.group == "empty"])
def test_gather_empty_regions(T, name):
    """Runs of empty regions in a gather and a fused gather, both forms."""
    run_case(T, name)


@pytest.mark.parametrize("name", [k for k, c in pec.CASES.items() if c.group == "unit"])
def test_unit_form_granule_edges(T, name):
    """The unit form's granule, unit and three-region edges under a roomy cap,
    and the same batches under a tight cap (the chunk form)."""
    run_case(T, name)
