"""Every entry that takes a caller workspace, run with a workspace of exactly the
advertised size cut from the middle of one filled tensor, guard | workspace |
guard: the status word is 0, every output equals what the same entry produced
just before with a generously oversized workspace (those outputs are checked
against the oracle elsewhere), and both guards still hold the fill -- so a
layout (kuma_amd/csrc/kmws_workspace.hpp) that places a region past the size it
advertises is seen here, inside one allocation, where nothing faults.  One byte
less is refused with the entry's status and leaves guards and workspace alone.

Shapes, the smallest at which a layout can still go wrong: five masked frames
of 0, 1, 20000, 16384 and 125 bytes in two streams (two full 16 KiB tiles and a
partial one) for the in-place entries and, by dst_cap alone, for both forms of
the copy entries; 2,049 frames of 0-3 bytes (past a 256-frame row and the
2,048-frame scan tile) for both forms of the copy entries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FILL = 0xA5
OUT_FILL = 0xEE
RELAY = (1 << 1) | (1 << 2)  # text and binary


@pytest.fixture(scope="module")
def T():
    import torch
    from kuma_amd import kmws
    if not torch.cuda.is_available() or kmws.device_count() < 1:
        pytest.fail("gpu test needs a gfx950 device")
    return torch


def r16(x):
    return (x + 15) // 16 * 16


def build_wire(lens, stream_first, seed):
    """A server-mode wire: FIN text frames, masked, printable ASCII payloads."""
    rng = np.random.default_rng(seed)
    parts, hdr_off, offs, keys, pos = [], [], [], [], 0
    for L in lens:
        key = int(rng.integers(1, 2 ** 32))
        hdr = [0x81, 0x80 | L] if L <= 125 else [0x81, 0x80 | 126, L >> 8, L & 0xFF]
        kb = np.frombuffer(key.to_bytes(4, "little"), dtype=np.uint8)
        plain = rng.integers(0x20, 0x7F, size=L, dtype=np.uint8)
        parts += [np.array(hdr, dtype=np.uint8), kb, plain ^ np.resize(kb, L)]
        hdr_off.append(pos)
        offs.append(pos + len(hdr) + 4)
        keys.append(key)
        pos += len(hdr) + 4 + L
    wire = np.concatenate(parts)
    return dict(wire=wire, total=pos, n=len(lens), lens=np.asarray(lens, dtype=np.int64),
                hdr_off=np.asarray(hdr_off, dtype=np.int64), offs=np.asarray(offs, dtype=np.int64),
                keys=np.asarray(keys, dtype=np.int64), stream_first=list(stream_first))


DATA = {
    "five": lambda: build_wire([0, 1, 20000, 16384, 125], [0, 2, 5], 14),
    "tiny": lambda: build_wire(list(np.random.default_rng(15).integers(0, 4, size=2049)), [0, 1000, 2049], 16),
}
_dev = {}


def data(T, name):
    """The batch on the device, built once per module."""
    from kuma_amd import kmws
    if name not in _dev:
        d = DATA[name]()
        n = d["n"]
        pad = r16(d["total"]) - d["total"] + 16
        d["d_wire"] = T.from_numpy(np.concatenate([d["wire"], np.zeros(pad, np.uint8)])).cuda()
        d["d_hdr_off"] = T.from_numpy(d["hdr_off"]).cuda()
        d["d_descs"] = kmws.make_descs(d["offs"], d["lens"], d["keys"])
        d["d_flags"] = T.full((n,), 0x81 | kmws.FLAG_MASK, dtype=T.int16, device="cuda")
        d["d_okeys"] = T.from_numpy(np.random.default_rng(17).integers(1, 2 ** 31, size=n).astype(np.int32)).cuda()
        d["d_sf"] = T.tensor(d["stream_first"], dtype=T.int32, device="cuda")
        d["ns"] = len(d["stream_first"]) - 1
        _dev[name] = d
    return _dev[name]


def cap_of(d, form):
    cap = r16(d["total"]) if form == "chunks" else d["n"] * 16384
    assert (cap // d["n"] < 16384) == (form == "chunks")
    return cap


class Outs:
    """Fresh, filled output tensors of one run, by name."""

    def __init__(self, T):
        self.T, self.t = T, {}

    def new(self, name, numel, dtype):
        fill = OUT_FILL if dtype == self.T.uint8 else -1
        self.t[name] = self.T.full((max(int(numel), 1),), fill, dtype=dtype, device="cuda")
        return self.t[name]

    def keep(self, name, tensor):
        self.t[name] = tensor
        return tensor

    def parsed(self, n):
        return (self.new("out_desc", 2 * n, self.T.int64).view(-1, 2)[:n], self.new("out_flags", n, self.T.int16),
                self.new("out_err", n, self.T.uint8))

    def streams(self, d):
        return dict(stream_first=d["d_sf"], carry_in=None, carry_out=self.new("carry_out", 8 * d["ns"], self.T.uint8))


# ---- the entries: size(kmws, d, cap) and run(kmws, L, d, cap, ws, o, small) ----
# `small`: the run is expected to be refused; a step that only prepares the
# workspace for the entry under test is left out then.
def _stream(T):
    return int(T.cuda.current_stream().cuda_stream)


def run_unmask_batch(kmws, T, d, cap, ws, o, small):
    base = o.keep("base", d["d_wire"].clone())
    kmws._check(kmws.lib().kmws_unmask_batch(base.data_ptr(), d["total"], d["d_descs"].data_ptr(), d["n"], ws.ptr,
                                             ws.nbytes, _stream(T)), "kmws_unmask_batch")


def run_unmask_plan(kmws, T, d, cap, ws, o, small):
    kmws.unmask_plan(d["d_descs"], ws, d["total"])
    o.keep("plan", ws.tensor[:kmws.unmask_workspace_size(d["total"])].clone())


def run_unmask_apply(kmws, T, d, cap, ws, o, small):
    base = o.keep("base", d["d_wire"].clone())
    if not small:
        kmws.unmask_plan(d["d_descs"], ws, d["total"])
    kmws._check(kmws.lib().kmws_unmask_apply(base.data_ptr(), d["total"], d["d_descs"].data_ptr(), d["n"], ws.ptr,
                                             ws.nbytes, _stream(T)), "kmws_unmask_apply")


def run_unmask_apply_sched(kmws, T, d, cap, ws, o, small):
    base = o.keep("base", d["d_wire"].clone())
    if not small:
        kmws.unmask_plan(d["d_descs"], ws, d["total"])
    kmws.unmask_apply(base, d["d_descs"], ws, d["total"], schedule=kmws.SCHED_SPLIT8 | kmws.SCHED_TEMPORAL_STORES)


def run_unpack_unmask(kmws, T, d, cap, ws, o, small):
    wire = o.keep("wire", d["d_wire"].clone())
    kmws.unpack_unmask(wire, d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), ws, wire_len=d["total"])


def run_utf8_validate(kmws, T, d, cap, ws, o, small):
    kmws.utf8_validate(d["d_wire"], d["d_descs"], d["d_flags"], o.new("out_utf8", d["n"], T.uint8), ws,
                       span=d["total"], masked=True, **o.streams(d))


def run_unmask_utf8(kmws, T, d, cap, ws, o, small):
    base = o.keep("base", d["d_wire"].clone())
    kmws.unmask_utf8(base, d["d_descs"], d["d_flags"], o.new("out_utf8", d["n"], T.uint8), ws, span=d["total"],
                     **o.streams(d))


def run_unpack_unmask_utf8(kmws, T, d, cap, ws, o, small):
    wire = o.keep("wire", d["d_wire"].clone())
    kmws.unpack_unmask_utf8(wire, d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), o.new("out_utf8", d["n"], T.uint8),
                            ws, wire_len=d["total"], **o.streams(d))


def run_pack_headers(kmws, T, d, cap, ws, o, small):
    n = d["n"]
    kmws.pack_headers(d["d_descs"], d["d_flags"], o.new("hdr", 16 * n, T.uint8), o.new("hdr_len", n, T.uint8),
                      o.new("wire_off", n + 1, T.int64), ws)


def run_unpack_headers(kmws, T, d, cap, ws, o, small):
    kmws.unpack_headers(d["d_wire"], d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), ws, wire_len=d["total"])


def run_encode(kmws, T, d, cap, ws, o, small):
    kmws.encode_batch(d["d_wire"], d["d_descs"], d["d_flags"], o.new("dst", cap, T.uint8),
                      o.new("off", d["n"] + 1, T.int64), ws)


def run_gather(kmws, T, d, cap, ws, o, small):
    kmws.gather_unmask(d["d_wire"], d["d_descs"], o.new("dst", cap, T.uint8), o.new("off", d["n"] + 1, T.int64), ws)


def run_unpack_gather(kmws, T, d, cap, ws, o, small):
    kmws.unpack_gather(d["d_wire"], d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), o.new("dst", cap, T.uint8),
                       o.new("off", d["n"] + 1, T.int64), ws, wire_len=d["total"])


def run_reframe(kmws, T, d, cap, ws, o, small):
    kmws.reframe_batch(d["d_wire"], d["d_descs"], d["d_flags"], d["d_okeys"], o.new("dst", cap, T.uint8),
                       o.new("off", d["n"] + 1, T.int64), ws)


def run_unpack_reframe(kmws, T, d, cap, ws, o, small):
    kmws.unpack_reframe(d["d_wire"], d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), RELAY, True, d["d_okeys"],
                        o.new("dst", cap, T.uint8), o.new("off", d["n"] + 1, T.int64), ws, wire_len=d["total"])


def run_gather_utf8(kmws, T, d, cap, ws, o, small):
    kmws.gather_unmask_utf8(d["d_wire"], d["d_descs"], d["d_flags"], o.new("dst", cap, T.uint8),
                            o.new("off", d["n"] + 1, T.int64), o.new("out_utf8", d["n"], T.uint8), ws, **o.streams(d))


def run_unpack_gather_utf8(kmws, T, d, cap, ws, o, small):
    kmws.unpack_gather_utf8(d["d_wire"], d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), o.new("dst", cap, T.uint8),
                            o.new("off", d["n"] + 1, T.int64), o.new("out_utf8", d["n"], T.uint8), ws,
                            wire_len=d["total"], **o.streams(d))


def run_reframe_utf8(kmws, T, d, cap, ws, o, small):
    kmws.reframe_utf8(d["d_wire"], d["d_descs"], d["d_flags"], d["d_okeys"], o.new("dst", cap, T.uint8),
                      o.new("off", d["n"] + 1, T.int64), o.new("out_utf8", d["n"], T.uint8), ws, **o.streams(d))


def run_unpack_reframe_utf8(kmws, T, d, cap, ws, o, small):
    kmws.unpack_reframe_utf8(d["d_wire"], d["d_hdr_off"], kmws.SERVER, *o.parsed(d["n"]), RELAY, True, d["d_okeys"],
                             o.new("dst", cap, T.uint8), o.new("off", d["n"] + 1, T.int64),
                             o.new("out_utf8", d["n"], T.uint8), ws, wire_len=d["total"], **o.streams(d))


def _plan(kmws, d, cap):
    return kmws.unmask_workspace_size(d["total"])


def _copy(kmws, d, cap):
    return kmws.copy_workspace_size(d["n"], cap)


IN_PLACE = {
    "kmws_unmask_batch": (_plan, run_unmask_batch),
    "kmws_unmask_plan": (_plan, run_unmask_plan),
    "kmws_unmask_apply": (_plan, run_unmask_apply),
    "kmws_unmask_apply_sched": (_plan, run_unmask_apply_sched),
    "kmws_unpack_unmask": (_plan, run_unpack_unmask),
    "kmws_utf8_validate": (lambda k, d, cap: k.utf8_workspace_size(d["total"], d["n"], d["ns"]), run_utf8_validate),
    "kmws_unmask_utf8_batch": (lambda k, d, cap: k.unmask_utf8_workspace_size(d["total"], d["n"], d["ns"]),
                               run_unmask_utf8),
    "kmws_unpack_unmask_utf8": (lambda k, d, cap: k.unmask_utf8_workspace_size(d["total"], d["n"], d["ns"]),
                                run_unpack_unmask_utf8),
    "kmws_unpack_headers": (lambda k, d, cap: k.lib().kmws_unpack_workspace_size(), run_unpack_headers),
}
HEADERS = {"kmws_pack_headers": (lambda k, d, cap: k.pack_headers_workspace_size(d["n"]), run_pack_headers)}
COPY = {
    "kmws_encode_batch": (_copy, run_encode),
    "kmws_gather_unmask": (_copy, run_gather),
    "kmws_unpack_gather": (_copy, run_unpack_gather),
    "kmws_reframe_batch": (lambda k, d, cap: k.reframe_workspace_size(d["n"], cap), run_reframe),
    "kmws_unpack_reframe": (lambda k, d, cap: k.reframe_workspace_size(d["n"], cap), run_unpack_reframe),
    "kmws_gather_unmask_utf8": (lambda k, d, cap: k.gather_utf8_workspace_size(d["n"], cap, d["ns"]), run_gather_utf8),
    "kmws_unpack_gather_utf8": (lambda k, d, cap: k.gather_utf8_workspace_size(d["n"], cap, d["ns"]),
                                run_unpack_gather_utf8),
    "kmws_reframe_utf8_batch": (lambda k, d, cap: k.reframe_utf8_workspace_size(d["n"], cap, d["ns"]),
                                run_reframe_utf8),
    "kmws_unpack_reframe_utf8": (lambda k, d, cap: k.reframe_utf8_workspace_size(d["n"], cap, d["ns"]),
                                 run_unpack_reframe_utf8),
}
CASES = ([(e, "five", None) for e in IN_PLACE] + [(e, b, None) for e in HEADERS for b in ("five", "tiny")] +
         [(e, b, f) for e in COPY for b in ("five", "tiny") for f in ("chunks", "units")])
ENTRIES = {**IN_PLACE, **HEADERS, **COPY}


def guarded_ws(T, kmws, size, take):
    """A workspace of `take` bytes at the start of the `size` bytes between two guards."""
    g = max(256, (size + 255) // 256 * 256)
    buf = T.full((g + size + g,), FILL, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace.__new__(kmws.Workspace)
    ws.tensor, ws.schedule = buf[g:g + take], None
    assert ws.ptr % 256 == 0 and ws.nbytes == take
    return buf, ws, g


@pytest.mark.parametrize("entry,batch,form", CASES, ids=[f"{e}-{b}-{f or 'inplace'}" for e, b, f in CASES])
def test_exact_workspace_keeps_its_guards(T, entry, batch, form):
    from kuma_amd import kmws
    size_of, run = ENTRIES[entry]
    d = data(T, batch)
    cap = cap_of(d, form) if form else 0
    size = size_of(kmws, d, cap)
    assert size >= 16

    big = kmws.Workspace(2 * size + 4096)
    big.tensor.fill_(FILL)
    want = Outs(T)
    run(kmws, T, d, cap, big, want, False)
    T.cuda.synchronize()
    assert big.status() == 0

    buf, ws, g = guarded_ws(T, kmws, size, size)
    got = Outs(T)
    run(kmws, T, d, cap, ws, got, False)
    T.cuda.synchronize()
    assert ws.status() == 0
    assert got.t.keys() == want.t.keys()
    for name in want.t:
        assert T.equal(got.t[name], want.t[name]), (entry, name)
    assert bool((buf[:g] == FILL).all()), "the guard below the workspace was written"
    assert bool((buf[g + size:] == FILL).all()), "the guard above the workspace was written"

    buf, ws, g = guarded_ws(T, kmws, size, size - 1)
    with pytest.raises(kmws.KmwsError) as e:
        run(kmws, T, d, cap, ws, Outs(T), True)
    T.cuda.synchronize()
    # kmws_unpack_headers has one status for a missing and a short workspace
    refused = kmws.ERR_INVALID_PARAM if entry == "kmws_unpack_headers" else kmws.ERR_BUFFER_TOO_SMALL
    assert e.value.status == refused
    assert bool((buf == FILL).all()), "a refused call wrote to the workspace or its guards"
