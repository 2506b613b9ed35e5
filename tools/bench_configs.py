#!/usr/bin/env python3
"""Secondary measurements for BASELINE.json configs 1, 3, 4 and the
end-to-end (host-memory) rate.  One JSON line per config on stdout.

  cfg1  1000 x 4 KiB masked TEXT frames, SERVER, fed in 64 KiB reads (runs
        bench.py --full --config cfg1: kuma's decoder restated in oracle/ as the CPU
        baseline, the product decoder and the batched send path).
  cfg3  Zipf 128 B-1 MiB, ~8 GiB payload, device-resident: encode (header pack
        + mask) -> unpack headers -> gather + unmask; round trip verified.
  cfg4  262,144 messages x 16 x 4 KiB fragments (FIN=0 chains), device-resident:
        header pack + mask, header unpack, in-place unmask; headers/s.
  e2e   host-resident 64 KiB-frame wire image (14-byte headers), in-place
        unmask through kmws_pipeline (pinned H2D -> kernel -> D2H).
  sync  the synchronous drop-in on kuma's call pattern, in C++
        (tests/cpp/sync_cfg1.cpp): cfg1 decoded per 64 KiB read and
        handleDataMask per send at 1/4/64 KiB, kuma's codec (oracle) vs the
        resident worker vs a launch per call.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x6B756D61


def splitmix_keys(seed, n):
    with np.errstate(over="ignore"):
        z = np.arange(n, dtype=np.uint64) + np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ------------------------------------------------------------------ cfg1
def cfg1(reps: int):
    """BASELINE configs[0]: lives in bench.py (`python bench.py --full --config cfg1`),
    whose cpu_baseline leg times kuma's decoder restated in oracle/."""
    sys.path.insert(0, ROOT)
    import bench
    return bench.run_cfg1(reps)


def sync(reps: int):
    """tests/cpp/sync_cfg1.cpp, built here with g++ against the product library
    and the oracle; its JSON lines gathered into one record."""
    import subprocess
    import tempfile
    from kuma_amd import build as kb
    from oracle import oracle as orc
    lib = kb.build()
    orc.build()
    odir = os.path.join(ROOT, "oracle")
    inc = os.path.join(ROOT, "include")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "sync_cfg1")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", inc, os.path.join(ROOT, "tests", "cpp", "sync_cfg1.cpp"),
                               "-L", os.path.dirname(lib), "-lkmws_gpu", "-L", odir, "-lkmws_oracle", "-lpthread",
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + odir, "-o", exe])
        r = subprocess.run([exe, str(reps)], capture_output=True, text=True, timeout=300)
    rows = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
    out = {"config": "sync", "rc": r.returncode, "cases": rows,
           "note": "in-process C++ driver, one codec call per 64 KiB read (decode) / per send (mask); "
                   "kuma_oracle = the oracle's restatement of kuma's codec on one core"}
    for x in rows:
        out.setdefault(x["case"], {}).setdefault(str(x.get("len", x.get("threads", "cfg1"))), {})[x["codec"]] = \
            x.get("GiB_s") if x["case"].startswith("decode_sync") else x.get("us_per_call")
    return out


def loopback(reps: int):
    """tests/cpp/loopback_cfg1.cpp over a real loopback socket (BASELINE
    configs[0]): kuma's codec (oracle) on both ends vs the synchronous member
    swap, the loop-batched gpu mode and the RxLoop adapter, 16 and 64 frames per
    send iteration; 1-8 connections at once; and the server alone (replay_*:
    clients replay a pre-built masked wire image, the server runs kuma's codec
    or the drop-in)."""
    import subprocess
    import tempfile
    from kuma_amd import build as kb
    from oracle import oracle as orc
    lib = kb.build()
    orc.build()
    odir = os.path.join(ROOT, "oracle")
    inc = os.path.join(ROOT, "include")
    rows = []
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "loopback_cfg1")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", inc, os.path.join(ROOT, "tests", "cpp", "loopback_cfg1.cpp"),
                               "-L", os.path.dirname(lib), "-lkmws_gpu", "-L", odir, "-lkmws_oracle", "-lpthread",
                               "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + odir, "-o", exe])
        for group in ("16", "64"):
            for mode, extra in (("cpu", []), ("sync", []), ("gpu", []), ("gpu", ["0", "noresident"]),
                                ("gpu", ["0", "submitpoll"]), ("adapter", []), ("adapter", ["0", "inflight2"]),
                                ("adapter", ["0", "ring16m"])):
                r = subprocess.run([exe, mode, str(reps), group] + extra, capture_output=True, text=True, timeout=300)
                got = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
                for x in got:
                    x["variant"] = extra[1] if extra else ""
                rows += got
        for mode in ("replay_cpu", "replay_adapter", "sink_cpu", "sink_adapter"):  # the server alone / the client alone
            r = subprocess.run([exe, mode, str(reps), "16"], capture_output=True, text=True, timeout=300)
            rows += [dict(json.loads(x), variant="") for x in r.stdout.strip().splitlines() if x.startswith("{")]
        for conns in ("2", "4", "8"):  # loop-thread pairs at once, 64 KiB per send iteration
            for mode in ("cpu", "sync", "gpu", "adapter", "replay_cpu", "replay_adapter", "sink_cpu", "sink_adapter"):
                r = subprocess.run([exe, mode, str(reps), "16", "0", "0", conns], capture_output=True, text=True,
                                   timeout=300)
                got = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
                for x in got:
                    x["variant"] = "conns" + conns
                rows += got
    out = {"config": "loopback_cfg1", "rows": rows}
    for x in rows:
        out.setdefault("GiB_s", {}).setdefault(str(x.get("frames_per_send_iteration")), {})[
            x["mode"] + ("_" + x["variant"] if x["variant"] else "")] = x.get("GiB_s")
    return out


# ------------------------------------------------------------------ cfg3
def zipf_lens(rng, n):
    k = np.arange(14)
    p = (k + 1.0) ** -1.2
    p /= p.sum()
    cls = rng.choice(14, size=n, p=p)
    return (128 * (2 ** cls) - rng.integers(0, 64, size=n)).astype(np.int64)


def verify_dense(torch, src, src_off, lens, dst, dst_off, frames_per_chunk=20000):
    """dst[dst_off[i] : +lens[i]] == src[src_off[i] : +lens[i]] for every frame, checked
    by an index gather in chunks (independent of the kernels under test)."""
    dev = src.device
    doff = dst_off.cpu().numpy()
    if not np.array_equal(doff[:-1], np.concatenate([[0], np.cumsum(lens)[:-1]])):
        return False
    for a in range(0, len(lens), frames_per_chunk):
        b = min(len(lens), a + frames_per_chunk)
        ln = torch.from_numpy(lens[a:b]).to(dev)
        so = torch.from_numpy(src_off[a:b].astype(np.int64)).to(dev)
        tot = int(ln.sum())
        if tot == 0:
            continue
        start = torch.repeat_interleave(so - (torch.cumsum(ln, 0) - ln), ln)
        idx = start + torch.arange(tot, device=dev)
        if not torch.equal(src[idx], dst[int(doff[a]):int(doff[a]) + tot]):
            return False
    return True


def placed_buffer(torch, kmws, span: int):
    """A device buffer of `span` bytes carved from a contiguous arena at the
    offset where the placement probe runs fastest (bench.place_batch, the
    headline bench's placement; DESIGN.md sec.4 'Placement of the batch').
    Returns (arena or None, uint8 view, placement record)."""
    import bench
    dev = torch.device("cuda", torch.cuda.current_device())
    arena, view, rec = bench.place_batch(kmws, torch, dev, span, 96 << 30)
    if arena is None:
        view = torch.empty(span, dtype=torch.uint8, device=dev)
    return arena, view, rec


def verify_sparse(torch, src, src_off, lens, dst, dst_off, frames_per_chunk=20000):
    """dst[dst_off[i] : +lens[i]] == src[src_off[i] : +lens[i]] for every frame (payloads
    where they lie, e.g. in a wire image), checked by index gathers in chunks."""
    dev = src.device
    for a in range(0, len(lens), frames_per_chunk):
        b = min(len(lens), a + frames_per_chunk)
        ln = torch.from_numpy(lens[a:b]).to(dev)
        tot = int(ln.sum())
        if tot == 0:
            continue
        rel = torch.arange(tot, device=dev) - torch.repeat_interleave(torch.cumsum(ln, 0) - ln, ln)
        so = torch.repeat_interleave(torch.from_numpy(src_off[a:b].astype(np.int64)).to(dev), ln)
        do = torch.repeat_interleave(torch.from_numpy(np.asarray(dst_off[a:b], dtype=np.int64)).to(dev), ln)
        if not torch.equal(src[so + rel], dst[do + rel]):
            return False
    return True


def timed(torch, fn, reps, calls=1):
    """Median over `reps` of the event-timed device time per call, `calls` calls
    back to back between the events (calls > 1 for operations of tens of us,
    whose single-call timing would include the Python binding's own time)."""
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3 / calls)
    ts.sort()
    return ts[len(ts) // 2]


def cfg3(reps: int, gib: float):
    import torch
    from kuma_amd import kmws
    rng = np.random.default_rng(SEED)
    lens = zipf_lens(rng, 4_000_000)
    cs = np.cumsum(lens)
    n = int(np.searchsorted(cs, gib * 2**30)) + 1
    lens = lens[:n]
    P = int(lens.sum())
    src_off = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.int64)
    src_bytes = int(src_off[-1] + lens[-1] + 16)
    flags = (0x80 | np.where(np.arange(n) % 2 == 0, 1, 2) | 0x100).astype(np.int16)
    keys = splitmix_keys(SEED ^ 3, n).astype(np.int64)
    dev = torch.device("cuda")
    src = torch.empty(src_bytes + 16, dtype=torch.uint8, device=dev)
    kmws.fill_synthetic(src, SEED)
    descs = kmws.make_descs(src_off, lens, keys)
    fl = torch.from_numpy(flags).to(dev)
    hl = np.where(lens <= 125, 2, np.where(lens <= 65535, 4, 10)) + 4
    H = int(hl.sum())
    wire = torch.empty(P + H + 16, dtype=torch.uint8, device=dev)
    wire_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_e = kmws.Workspace(kmws.copy_workspace_size(n, wire.numel()))
    t_enc = timed(torch, lambda: kmws.encode_batch(src, descs, fl, wire, wire_off, ws_e), reps, calls=3)
    assert ws_e.status() == 0 and int(wire_off[n]) == P + H
    # decode: descriptor-indexed (header offsets as a receiver's host parser hands them over)
    hdr_off = wire_off[:n]
    out_desc = torch.empty((n, 2), dtype=torch.int64, device=dev)
    out_flags = torch.empty(n, dtype=torch.int16, device=dev)
    out_err = torch.empty(n, dtype=torch.uint8, device=dev)
    ws_u = kmws.Workspace(16)
    dst = torch.empty(P + 16, dtype=torch.uint8, device=dev)
    dst_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_g = kmws.Workspace(kmws.copy_workspace_size(n, dst.numel()))

    def decode():
        kmws.unpack_headers(wire, hdr_off, kmws.SERVER, out_desc, out_flags, out_err, ws_u, wire_len=P + H)
        kmws.gather_unmask(wire, out_desc, dst, dst_off, ws_g)

    t_dec = timed(torch, decode, reps, calls=3)
    # the same decode with the header parse fused into the gather's scan (kmws_unpack_gather)
    dst_f = torch.empty(P + 16, dtype=torch.uint8, device=dev)
    dst_off_f = torch.empty(n + 1, dtype=torch.int64, device=dev)
    od_f = torch.empty((n, 2), dtype=torch.int64, device=dev)
    ws_gf = kmws.Workspace(kmws.copy_workspace_size(n, dst_f.numel()))
    t_dec_f = timed(torch, lambda: kmws.unpack_gather(wire, hdr_off, kmws.SERVER, od_f, None, None, dst_f, dst_off_f,
                                                      ws_gf, wire_len=P + H), reps, calls=3)
    t_unpack = timed(torch, lambda: kmws.unpack_headers(wire, hdr_off, kmws.SERVER, out_desc, out_flags,
                                                        out_err, ws_u, wire_len=P + H), reps, calls=20)
    assert ws_u.status() == 0 and ws_g.status() == 0 and int(out_err.max()) == 0
    # round trip: every byte of the dense output == the source payloads
    ok = verify_dense(torch, src, src_off, lens, dst, dst_off)
    enc_bytes = 2 * P + H + 26 * n
    dec_bytes = 2 * P + H + 51 * n
    # decode in place, as kuma does (WSHandler.cpp:247-250): unpack, then unmask the
    # payloads where they lie in the wire (kmws_unmask_batch on the unpacked descriptors)
    ws_m = kmws.Workspace(kmws.unmask_workspace_size(P + H))
    sched = kmws.unmask_autotune(wire, out_desc, ws_m, P + H)  # this batch's schedule (payload unchanged)
    kmws.unmask_batch(wire, out_desc, ws_m, P + H)  # one pass: unmasked, verified below
    torch.cuda.synchronize()
    ok_in_place = ws_m.status() == 0 and verify_sparse(torch, src, src_off, lens, wire, out_desc[:, 0].cpu().numpy())
    t_unmask = timed(torch, lambda: kmws.unmask_batch(wire, out_desc, ws_m, P + H), 2 * (reps // 2) + 2)

    def decode_in_place():
        kmws.unpack_headers(wire, hdr_off, kmws.SERVER, out_desc, out_flags, out_err, ws_u, wire_len=P + H)
        kmws.unmask_batch(wire, out_desc, ws_m, P + H)

    t_dip = timed(torch, decode_in_place, 2 * (reps // 2) + 2)  # even: the wire stays unmasked
    # fused: header parse writing the unmask plan, then the apply (kmws_unpack_unmask)
    ws_mf = kmws.Workspace(kmws.unmask_workspace_size(P + H))
    ws_mf.schedule = sched
    t_dip_f = timed(torch, lambda: kmws.unpack_unmask(wire, hdr_off, kmws.SERVER, od_f, None, None, ws_mf,
                                                      wire_len=P + H), 2 * (reps // 2) + 2)  # even
    kmws.unmask_batch(wire, out_desc, ws_m, P + H)  # back to the masked wire image
    torch.cuda.synchronize()
    ok_fused = (ws_gf.status() == 0 and ws_mf.status() == 0 and torch.equal(od_f, out_desc) and
                torch.equal(dst_off_f, dst_off) and torch.equal(dst_f[:P], dst[:P]))
    ok = ok and ok_in_place and ok_fused
    # encode in kuma's iovec form (sendWsFrame, WebSocketImpl.cpp:381-436): headers packed into
    # 16-B slots (kmws_pack_headers), payloads masked in place where they lie (kmws_unmask_batch)
    hslots = torch.empty(16 * n, dtype=torch.uint8, device=dev)
    hlen = torch.empty(n, dtype=torch.uint8, device=dev)
    woff2 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_h = kmws.Workspace(kmws.pack_headers_workspace_size(n))
    ws_s = kmws.Workspace(kmws.unmask_workspace_size(src_bytes))
    sched_s = kmws.unmask_autotune(src, descs, ws_s, src_bytes)

    def encode_iovec():
        kmws.pack_headers(descs, fl, hslots, hlen, woff2, ws_h)
        kmws.unmask_batch(src, descs, ws_s, src_bytes)

    encode_iovec()  # one pass: every payload masked in place -> equal to the wire image's payloads
    torch.cuda.synchronize()
    woff_h = wire_off.cpu().numpy()
    ok_iov = (ws_s.status() == 0 and torch.equal(woff2, wire_off) and
              verify_sparse(torch, wire, woff_h[:n] + hl, lens, src, src_off) and            # masked payloads
              verify_sparse(torch, wire, woff_h[:n], hl.astype(np.int64), hslots, 16 * np.arange(n)))  # headers
    t_iov = timed(torch, encode_iovec, 2 * (reps // 2) + 1)  # odd: the payloads end unmasked, as they started
    ok = ok and ok_iov
    return {"config": "cfg3", "frames": n, "payload_bytes": P, "header_bytes": H,
            "encode": {"ms": t_enc * 1e3, "payload_GiB_s": P / t_enc / 2**30,
                       "alg_GB_s": enc_bytes / t_enc / 1e9, "hbm_frac": enc_bytes / t_enc / 8e12},
            "decode_unpack_gather": {"ms": t_dec * 1e3, "payload_GiB_s": P / t_dec / 2**30,
                                     "alg_GB_s": dec_bytes / t_dec / 1e9, "hbm_frac": dec_bytes / t_dec / 8e12},
            "decode_unpack_gather_fused": {"ms": t_dec_f * 1e3, "payload_GiB_s": P / t_dec_f / 2**30,
                                           "alg_GB_s": dec_bytes / t_dec_f / 1e9,
                                           "hbm_frac": dec_bytes / t_dec_f / 8e12,
                                           "note": "kmws_unpack_gather: header parse inside the gather's scan"},
            "unpack_only": {"ms": t_unpack * 1e3, "Mheaders_s": n / t_unpack / 1e6},
            "encode_iovec_in_place": {"ms": t_iov * 1e3, "payload_GiB_s": P / t_iov / 2**30, "schedule": sched_s,
                                      "hbm_frac": (2 * P + 59 * n) / t_iov / 8e12,
                                      "note": "kmws_pack_headers (16-B header slots) + in-place mask of the payloads"},
            "unmask_in_place": {"ms": t_unmask * 1e3, "payload_GiB_s": P / t_unmask / 2**30, "schedule": sched,
                                "hbm_frac": (2 * P + 16 * n) / t_unmask / 8e12},
            "decode_unpack_in_place": {"ms": t_dip * 1e3, "payload_GiB_s": P / t_dip / 2**30,
                                       "hbm_frac": (2 * P + H + 16 * n + 35 * n) / t_dip / 8e12},
            "decode_unpack_in_place_fused": {"ms": t_dip_f * 1e3, "payload_GiB_s": P / t_dip_f / 2**30,
                                             "hbm_frac": (2 * P + H + 16 * n + 35 * n) / t_dip_f / 8e12,
                                             "note": "kmws_unpack_unmask: parse + plan in one kernel, then apply"},
            "verified_fused": bool(ok_fused),
            "roundtrip_payload_GiB_s": P / (t_enc + t_dec) / 2**30, "verified": bool(ok),
            "note": "decode is descriptor-indexed: header offsets = the receiver's host parse (here wire_off)"}


class PinnedHost:
    """Exactly nbytes of page-locked host memory: numpy pages (touched, so they
    are resident) registered with hipHostRegister.  torch's pin_memory() would
    round the request up to a power of two in its caching host allocator (two
    8 GiB buffers become 32 GiB pinned).  close() unregisters BEFORE the numpy
    pages are released: a registration outliving its pages would make the
    runtime treat a later allocation at the same addresses as pinned and DMA
    through the stale mapping (an illegal-address fault on the next H2D copy)."""

    def __init__(self, torch, nbytes: int):
        self._rt = torch.cuda.cudart()
        self.array = np.empty(nbytes, dtype=np.uint8)
        self.array.fill(0)
        if int(self._rt.cudaHostRegister(self.array.ctypes.data, nbytes, 0)) != 0:
            raise RuntimeError("hipHostRegister failed")
        self.tensor = torch.from_numpy(self.array)
        assert self.tensor.is_pinned()

    def close(self):
        if self.array is not None:
            self.tensor = None
            if int(self._rt.cudaHostUnregister(self.array.ctypes.data)) != 0:
                raise RuntimeError("hipHostUnregister failed")
            self.array = None


def cfg3_e2e(gib: float, chunk_mib: int, reps: int):
    """BASELINE configs[2] end to end (SURVEY 8 d row 3 ii): a pinned host
    buffer of plain Zipf payloads (dense, back to back) -> per chunk of frames
    (<= chunk_mib of payload): H2D -> kmws_encode_batch (header pack + mask) ->
    kmws_unpack_headers -> kmws_gather_unmask -> D2H into a second pinned host
    buffer, which must equal the input.  Three slots on three streams (H2D ||
    device work || D2H, ordered by events), as kmws_pipeline's ring."""
    import torch
    from kuma_amd import kmws
    rng = np.random.default_rng(SEED ^ 0xE2E)
    lens = zipf_lens(rng, 4_000_000)
    n = int(np.searchsorted(np.cumsum(lens), gib * 2**30)) + 1
    lens = lens[:n]
    P = int(lens.sum())
    pay_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)  # dense host layout
    flags = (0x80 | np.where(np.arange(n) % 2 == 0, 1, 2) | 0x100).astype(np.int16)
    keys = splitmix_keys(SEED ^ 5, n).astype(np.int64)
    hl = np.where(lens <= 125, 2, np.where(lens <= 65535, 4, 10)) + 4
    # chunks of whole frames, <= chunk bytes of payload each; source offsets relative
    # to the chunk's 16-B aligned host start
    cb = chunk_mib << 20
    cuts = [0]
    while cuts[-1] < n:
        a = cuts[-1]
        cuts.append(max(a + 1, int(np.searchsorted(pay_off, pay_off[a] + cb, side="right")) - 1))
    cuts[-1] = n
    chunks = []
    rel = np.empty(n, dtype=np.int64)
    for a, b in zip(cuts, cuts[1:]):
        h0 = int(pay_off[a]) & ~15
        rel[a:b] = pay_off[a:b] - h0
        chunks.append((a, b, h0, int(pay_off[b]) - h0, int(pay_off[b] - pay_off[a]), int((hl[a:b] + lens[a:b]).sum())))
    torch.cuda.synchronize()
    pin_src, pin_dst = PinnedHost(torch, P + 32), PinnedHost(torch, P + 32)
    try:
        return _cfg3_e2e_run(torch, kmws, pin_src.tensor, pin_dst.tensor, P, n, lens, pay_off, rel, flags, keys,
                             chunks, cb, chunk_mib, reps)
    finally:
        torch.cuda.synchronize()  # no copy still reading or writing the pages
        pin_src.close()
        pin_dst.close()


def _cfg3_e2e_run(torch, kmws, host_src, host_dst, P, n, lens, pay_off, rel, flags, keys, chunks, cb, chunk_mib,
                  reps):
    dev = torch.device("cuda")
    tmp = torch.empty(P + 32, dtype=torch.uint8, device=dev)
    kmws.fill_synthetic(tmp, SEED ^ 9)
    host_src.copy_(tmp)
    del tmp
    host_dst.zero_()
    descs = kmws.make_descs(rel, lens, keys)
    fl = torch.from_numpy(flags).to(dev)
    nmax = max(b - a for a, b, *_ in chunks)
    spanmax = max(c[3] for c in chunks)
    wmax = max(c[5] for c in chunks)
    S = 3
    slots = []
    for _ in range(S):
        slots.append({
            "src": torch.empty(spanmax + 32, dtype=torch.uint8, device=dev),
            "wire": torch.empty(wmax + 32, dtype=torch.uint8, device=dev),
            "dst": torch.empty(cb + 32, dtype=torch.uint8, device=dev),
            "wire_off": torch.empty(nmax + 1, dtype=torch.int64, device=dev),
            "out_desc": torch.empty((nmax, 2), dtype=torch.int64, device=dev),
            "dst_off": torch.empty(nmax + 1, dtype=torch.int64, device=dev),
            "ws_e": kmws.Workspace(kmws.copy_workspace_size(nmax, wmax + 32)),
            "ws_u": kmws.Workspace(16),
            "ws_g": kmws.Workspace(kmws.copy_workspace_size(nmax, cb + 32)),
            "h2d": torch.cuda.Event(), "comp": torch.cuda.Event(), "d2h": torch.cuda.Event(),
        })
    s_h2d, s_comp, s_d2h = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(chunks) + 1)]
    issue = [0.0]
    torch.cuda.synchronize()

    def one_pass():
        marks[0].record(s_d2h)
        for c, (a, b, h0, span, pc, wc) in enumerate(chunks):
            sl = slots[c % S]
            nc = b - a
            if c >= S:
                # the slot's previous chunk has left the device: a host wait keeps at most S
                # chunks of work queued (a deep queue of cross-stream waits stalled the copies)
                sl["d2h"].synchronize()
            with torch.cuda.stream(s_h2d):
                sl["src"][:span].copy_(host_src[h0:h0 + span], non_blocking=True)
                sl["h2d"].record(s_h2d)
            s_comp.wait_event(sl["h2d"])
            kmws.encode_batch(sl["src"], descs[a:b], fl[a:b], sl["wire"], sl["wire_off"][:nc + 1], sl["ws_e"],
                              stream=s_comp)
            kmws.unpack_headers(sl["wire"], sl["wire_off"][:nc], kmws.SERVER, sl["out_desc"][:nc], None, None,
                                sl["ws_u"], wire_len=wc, stream=s_comp)
            kmws.gather_unmask(sl["wire"], sl["out_desc"][:nc], sl["dst"], sl["dst_off"][:nc + 1], sl["ws_g"],
                               stream=s_comp)
            sl["comp"].record(s_comp)
            with torch.cuda.stream(s_d2h):
                s_d2h.wait_event(sl["comp"])
                host_dst[int(pay_off[a]):int(pay_off[b])].copy_(sl["dst"][:pc], non_blocking=True)
                sl["d2h"].record(s_d2h)
                marks[c + 1].record(s_d2h)
        issue[0] = time.perf_counter()
        torch.cuda.synchronize()

    one_pass()  # warm
    ok = bool(torch.equal(host_dst[:P], host_src[:P]))
    st = [sl[w].status() for sl in slots for w in ("ws_e", "ws_u", "ws_g")]
    best, issue_s = 1e9, 0.0
    for _ in range(reps):
        host_dst[:P].zero_()
        t0 = time.perf_counter()
        one_pass()
        t1 = time.perf_counter()
        if t1 - t0 < best:
            best, issue_s = t1 - t0, issue[0] - t0
    ok = ok and bool(torch.equal(host_dst[:P], host_src[:P])) and not any(st)
    gaps = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(len(chunks)))  # last pass, ms per chunk
    qs = {q: round(gaps[int(q * (len(gaps) - 1))], 3) for q in (0.1, 0.5, 0.9)}
    return {"config": "cfg3_e2e", "frames": n, "payload_bytes": P, "chunks": len(chunks), "chunk_MiB": chunk_mib,
            "slots": S, "payload_GiB_s": P / best / 2**30, "pcie_bytes": 2 * P, "verified": ok,
            "chunk_ms_quantiles": qs, "host_issue_s": round(issue_s, 4), "total_s": round(best, 4),
            "note": "pinned host plain payload -> H2D -> encode (pack+mask) -> unpack -> gather-unmask -> D2H, "
                    "3 slots on 3 streams; PCIe-bound (each payload byte crosses twice)"}


def cfg2b(reps: int, frames: int, placed: bool = True, header: int = 14):
    """BASELINE configs[1] variant B (SURVEY 8 d row 2): the same 1 M x 64 KiB
    frames as a packed wire image -- 14-byte masked headers between payloads,
    so payload starts are misaligned (payload f at 14 + f * 65,550) -- unmasked
    in place on the device.  Tiles holding a frame boundary take the general
    (descriptor-staged, byte-exact) path; headers keep their bytes."""
    import torch
    from kuma_amd import kmws
    L, H = 65536, header
    n = frames
    span = n * (L + H)
    dev = torch.device("cuda")
    wire = torch.empty(span, dtype=torch.uint8, device=dev)
    kmws.fill_synthetic(wire, SEED)
    descs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    kmws.fill_uniform_descs(descs, L + H, L, SEED ^ 7)
    descs[:, 0] += H
    ws = kmws.Workspace(kmws.unmask_workspace_size(span))
    alg = n * (2 * L + 16)

    def run(buf, tune=True):
        sched = kmws.unmask_autotune(buf, descs, ws, span) if tune else kmws.unmask_get_schedule(ws, descs, span)
        kmws.unmask_batch(buf, descs, ws, span)  # odd number of passes in total: verify the masked state
        t = timed(torch, lambda: kmws.unmask_batch(buf, descs, ws, span), 2 * (reps // 2) + 2)  # even: back to masked
        ok = ws.status() == 0 and kmws.check_unmasked(buf, SEED, descs) == 0
        if ok:
            kmws.unmask_batch(buf, descs, ws, span)  # back to the generated (masked) state
        return sched, t, bool(ok)

    # an aligned batch tuned first in the same process (it picks
    # temporal stores on most boxes) must leave this wire on the default
    # schedule, whose automatic store policy is non-temporal for it
    na = 16384
    abuf = torch.empty(na * L, dtype=torch.uint8, device=dev)
    adescs = torch.empty((na, 2), dtype=torch.int64, device=dev)
    kmws.fill_synthetic(abuf, SEED)
    kmws.fill_uniform_descs(adescs, L, L, SEED ^ 9)
    aws = kmws.Workspace(kmws.unmask_workspace_size(na * L))
    aligned_sched = kmws.unmask_autotune(abuf, adescs, aws, na * L)
    del abuf
    torch.cuda.empty_cache()
    sched_d, t_d, ok_d = run(wire, tune=False)
    sched, t, ok = run(wire)
    ok = ok and ok_d
    res = {"config": "cfg2b", "frames": n, "frame_len": L, "header_len": H, "span_bytes": span,
           "schedule": sched, "ms": t * 1e3, "payload_GiB_s": n * L / t / 2**30,
           "alg_GB_s": alg / t / 1e9, "hbm_frac": alg / t / 8e12, "verified": ok,
           "default_after_aligned_autotune": {"aligned_batch_schedule": aligned_sched, "schedule": sched_d,
                                              "ms": t_d * 1e3, "hbm_frac": alg / t_d / 8e12},
           "note": "device-resident packed wire (14-B headers, misaligned payloads), in-place unmask, plan + apply; "
                   "top level: plain torch.empty wire; 'placed': the same wire in a probed arena like bench.py"}
    if placed:
        del wire
        torch.cuda.empty_cache()
        arena, buf, rec = placed_buffer(torch, kmws, span)
        kmws.fill_synthetic(buf, SEED)
        sched, t, ok = run(buf)
        res["placed"] = {"schedule": sched, "ms": t * 1e3, "payload_GiB_s": n * L / t / 2**30,
                         "hbm_frac": alg / t / 8e12, "verified": ok, "placement": rec}
        del buf, arena
        res["verified"] = res["verified"] and ok
    return res


# ------------------------------------------------------------------ cfg4
def cfg4(reps: int, messages: int, placed: bool = True):
    import torch
    from kuma_amd import kmws
    n, L = messages * 16, 4096
    P = n * L
    dev = torch.device("cuda")
    src = torch.empty(P + 16, dtype=torch.uint8, device=dev)
    kmws.fill_synthetic(src, SEED)
    descs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    kmws.fill_uniform_descs(descs, L, L, SEED ^ 4)
    pos = np.arange(16)
    b0 = np.where(pos == 0, 1, 0) | np.where(pos == 15, 0x80, 0)   # TEXT/CONT chain (a-12)
    fl16 = torch.from_numpy(np.tile((b0 | 0x100).astype(np.int16), messages)).to(dev)
    fl16[0::32] = 0x100 | 1
    fl16[16::32] = 0x100 | 2                                        # alternate TEXT / BINARY messages
    H = n * 8
    wire = torch.empty(P + H + 16, dtype=torch.uint8, device=dev)
    wire_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_e = kmws.Workspace(kmws.copy_workspace_size(n, wire.numel()))
    t_pack = timed(torch, lambda: kmws.encode_batch(src, descs, fl16, wire, wire_off, ws_e), reps, calls=3)
    assert ws_e.status() == 0 and int(wire_off[n]) == P + H
    # headers only (kmws_pack_headers: 16-B slots + lengths + wire offsets), the iovec send form
    hslots = torch.empty(16 * n, dtype=torch.uint8, device=dev)
    hlen = torch.empty(n, dtype=torch.uint8, device=dev)
    woff2 = torch.empty(n + 1, dtype=torch.int64, device=dev)
    ws_h = kmws.Workspace(kmws.pack_headers_workspace_size(n))
    t_hdr = timed(torch, lambda: kmws.pack_headers(descs, fl16, hslots, hlen, woff2, ws_h, check=False), reps,
                  calls=20)
    assert torch.equal(woff2, wire_off) and torch.equal(hslots.view(n, 16)[:, :8], wire[:P + H].view(n, L + 8)[:, :8])
    # encode in kuma's iovec form: the header-only pack + the fragments masked in place where they lie
    ws_s = kmws.Workspace(kmws.unmask_workspace_size(P))
    sched_s = kmws.unmask_autotune(src, descs, ws_s, P)

    def encode_iovec():
        kmws.pack_headers(descs, fl16, hslots, hlen, woff2, ws_h)
        kmws.unmask_batch(src, descs, ws_s, P)

    encode_iovec()  # one pass: fragments masked, equal to the wire image's payloads
    torch.cuda.synchronize()
    ok_iov = ws_s.status() == 0 and bool(torch.equal(src[:P].view(n, L), wire[:P + H].view(n, L + 8)[:, 8:]))
    t_iov = timed(torch, encode_iovec, 2 * (reps // 2) + 1)  # odd: the fragments end unmasked, as they started
    out_desc = torch.empty((n, 2), dtype=torch.int64, device=dev)
    out_flags = torch.empty(n, dtype=torch.int16, device=dev)
    out_err = torch.empty(n, dtype=torch.uint8, device=dev)
    ws_u = kmws.Workspace(16)
    hdr_off = wire_off[:n]
    t_unpack = timed(torch, lambda: kmws.unpack_headers(wire, hdr_off, kmws.SERVER, out_desc, out_flags, out_err,
                                                        ws_u, wire_len=P + H), reps, calls=20)
    assert int(out_err.max()) == 0
    assert torch.equal(out_flags.cpu(), fl16.cpu())
    ws_m = kmws.Workspace(kmws.unmask_workspace_size(P + H))
    sched = kmws.unmask_autotune(wire, out_desc, ws_m, P + H)  # this batch's schedule (payload unchanged)
    kmws.unmask_batch(wire, out_desc, ws_m, P + H)   # once, then verify, then time pairs (identity)
    torch.cuda.synchronize()
    w = wire[:P + H].view(n, L + 8)[:, 8:]
    verified = bool(torch.equal(w.reshape(-1), src[:P]))
    # odd whatever --reps: the wire ends masked again, the state the placed copy
    # below starts from (its odd pass count then leaves it unmasked)
    t_unmask = timed(torch, lambda: kmws.unmask_batch(wire, out_desc, ws_m, P + H), 2 * (reps // 2) + 1)
    # the descriptor-indexed decode in place: two-step (unpack + unmask) and fused (kmws_unpack_unmask)
    t_dip = timed(torch, lambda: (kmws.unpack_headers(wire, hdr_off, kmws.SERVER, out_desc, out_flags, out_err,
                                                      ws_u, wire_len=P + H),
                                  kmws.unmask_batch(wire, out_desc, ws_m, P + H)), 2 * (reps // 2) + 2)  # even
    od_f = torch.empty((n, 2), dtype=torch.int64, device=dev)
    ws_mf = kmws.Workspace(kmws.unmask_workspace_size(P + H))
    ws_mf.schedule = sched
    t_dip_f = timed(torch, lambda: kmws.unpack_unmask(wire, hdr_off, kmws.SERVER, od_f, None, None, ws_mf,
                                                      wire_len=P + H), 2 * (reps // 2) + 2)  # even
    torch.cuda.synchronize()
    ok_fused = ws_mf.status() == 0 and bool(torch.equal(od_f, out_desc))
    verified = verified and ok_fused
    placed_rec = None
    if placed:  # the same in-place unmask on a copy of the wire in a placement-probed arena (as bench.py)
        arena, pw, rec = placed_buffer(torch, kmws, P + H)
        pw.copy_(wire[:P + H])
        sched_p = kmws.unmask_autotune(pw, out_desc, ws_m, P + H)
        t_p = timed(torch, lambda: kmws.unmask_batch(pw, out_desc, ws_m, P + H), 2 * (reps // 2) + 1)  # odd
        torch.cuda.synchronize()
        ok_p = ws_m.status() == 0 and bool(torch.equal(pw.view(n, L + 8)[:, 8:].reshape(-1), src[:P]))
        placed_rec = {"ms": t_p * 1e3, "payload_GiB_s": P / t_p / 2**30, "schedule": sched_p,
                      "hbm_frac": (2 * P + 16 * n) / t_p / 8e12, "verified": ok_p, "placement": rec}
        verified = verified and ok_p
        del pw, arena
    # device boundary discovery: the wire cut into S streams at message boundaries, one lane per stream
    walk = {}
    for S in (4096, 65536):
        per = n // S
        soff = torch.cat([wire_off[0:n:per], wire_off[n:n + 1]]).contiguous()
        hdr_w, n_w, _ = kmws.find_headers_streams(wire, soff, per, wire_len=P + H)
        t_w = timed(torch, lambda: kmws.find_headers_streams(wire, soff, per, wire_len=P + H), reps)
        assert int(n_w.sum()) == n and torch.equal(hdr_w.reshape(-1), wire_off[:n])
        walk[str(S)] = {"frames_per_stream": per, "ms": t_w * 1e3, "Mheaders_s": n / t_w / 1e6}
    # host boundary discovery rate (the serial part a receiver runs as bytes arrive), 1 GiB sample
    sample = wire[:min(P + H, 1 << 30)].cpu().numpy()
    out = np.zeros(sample.nbytes // 2 + 1, dtype=np.uint64)
    t_walk = 1e9
    for _ in range(3):  # the C walk only (no copies, no list conversion), best of 3
        t0 = time.perf_counter()
        nh, _ = kmws.find_headers_into(sample, out)
        t_walk = min(t_walk, time.perf_counter() - t0)
    hdrs = out[:nh]
    return {"config": "cfg4", "messages": messages, "frames": n, "payload_bytes": P,
            "pack": {"ms": t_pack * 1e3, "Mheaders_s": n / t_pack / 1e6, "payload_GiB_s": P / t_pack / 2**30,
                     "hbm_frac": (2 * P + H + 26 * n) / t_pack / 8e12},
            "encode_iovec_in_place": {"ms": t_iov * 1e3, "Mheaders_s": n / t_iov / 1e6, "schedule": sched_s,
                                      "payload_GiB_s": P / t_iov / 2**30, "hbm_frac": (2 * P + 59 * n) / t_iov / 8e12,
                                      "verified": ok_iov},
            "pack_headers_only": {"ms": t_hdr * 1e3, "Mheaders_s": n / t_hdr / 1e6,
                                  # desc 16 + flags 2 in, slot 16 + length 1 + wire offset 8 out
                                  "hbm_frac": 43 * n / t_hdr / 8e12, "timing": "20 calls back to back per event pair"},
            "unpack": {"ms": t_unpack * 1e3, "Mheaders_s": n / t_unpack / 1e6},
            "decode_unpack_in_place": {"ms": t_dip * 1e3, "payload_GiB_s": P / t_dip / 2**30,
                                       "hbm_frac": (2 * P + H + 51 * n) / t_dip / 8e12},
            "decode_unpack_in_place_fused": {"ms": t_dip_f * 1e3, "payload_GiB_s": P / t_dip_f / 2**30,
                                             "hbm_frac": (2 * P + H + 51 * n) / t_dip_f / 8e12,
                                             "note": "kmws_unpack_unmask: parse + plan in one kernel, then apply"},
            "unmask_in_place": {"ms": t_unmask * 1e3, "payload_GiB_s": P / t_unmask / 2**30, "schedule": sched,
                                "hbm_frac": (2 * P + 16 * n) / t_unmask / 8e12, "placed": placed_rec},
            "host_header_walk": {"frames": len(hdrs), "Mheaders_s": len(hdrs) / t_walk / 1e6},
            "device_header_walk_by_streams": walk,
            "verified_parts": {"unmask_in_place": verified, "encode_iovec": ok_iov,
                               "placed": placed_rec["verified"] if placed_rec else None},
            "verified": verified and ok_iov}


# ------------------------------------------------------------------ e2e
def e2e(gib: float, chunk_mib: int, depth: int):
    import torch
    from kuma_amd import kmws
    L = 65536
    n = int(gib * 2**30 // (L + 14))
    span = n * (L + 14)
    host = torch.empty(span, dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    offs = np.arange(n, dtype=np.uint64) * (L + 14) + 14
    d = np.zeros(n, dtype=[("off", "<u8"), ("len", "<u4"), ("key", "<u4")])
    d["off"], d["len"], d["key"] = offs, L, splitmix_keys(SEED, n)
    hv[:] = 0x5A
    rates = {}
    for name, mode in (("zerocopy", kmws.Pipeline.ZEROCOPY), ("sdma_ring", kmws.Pipeline.COPY)):
        p = kmws.Pipeline(0, chunk_mib << 20, 1 << 16, depth, transfer=mode)
        p.unmask(host, d)  # warm
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            p.unmask(host, d)
            ts.append(time.perf_counter() - t0)
        rates[name] = n * L / sorted(ts)[1] / 2**30
        del p
    t = n * L / max(rates.values()) / 2**30
    # 2 modes x (1 warm + 3) = 8 passes: even, so every byte (payloads, headers,
    # the 16-B hulls the zero-copy kernel rewrites) is back to 0x5A
    ok = bool((host == 0x5A).all())
    # raw PCIe copies for context
    cb = min(1 << 30, span)
    dbuf = torch.empty(cb, dtype=torch.uint8, device="cuda")
    hb = host[:cb]
    torch.cuda.synchronize()
    t0 = time.perf_counter(); dbuf.copy_(hb, non_blocking=True); torch.cuda.synchronize(); h2d = cb / (time.perf_counter() - t0)
    t0 = time.perf_counter(); hb.copy_(dbuf, non_blocking=True); torch.cuda.synchronize(); d2h = cb / (time.perf_counter() - t0)
    return {"config": "e2e", "frames": n, "frame_len": L, "host_bytes": span, "chunk_MiB": chunk_mib,
            "depth": depth, "payload_GiB_s": n * L / t / 2**30, "by_transfer_GiB_s": rates,
            "pcie_h2d_GiB_s": h2d / 2**30, "pcie_d2h_GiB_s": d2h / 2**30, "verified": ok,
            "note": "pinned host wire image, in-place unmask: zero-copy kernel over PCIe vs 3-slot SDMA H2D/kernel/D2H ring"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", nargs="+", choices=["cfg1", "cfg2b", "cfg3", "cfg3_e2e", "cfg4", "e2e", "sync", "loopback"])
    ap.add_argument("--cfg2b-frames", type=int, default=1 << 20)
    ap.add_argument("--cfg2b-header", type=int, default=14, help="bytes between payloads (14 = masked 64 KiB header)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--placement", default="probe", choices=["probe", "plain"],
                    help="probe: cfg2b and cfg4's in-place unmask also run in a placement-probed arena, as bench.py")
    ap.add_argument("--cfg3-gib", type=float, default=8.0)
    ap.add_argument("--cfg4-messages", type=int, default=262144)
    ap.add_argument("--e2e-gib", type=float, default=8.0)
    ap.add_argument("--e2e-chunk-mib", type=int, default=64)
    ap.add_argument("--e2e-depth", type=int, default=3)
    a = ap.parse_args()
    for w in a.which:
        if w == "cfg1":
            r = cfg1(max(a.reps, 10))
        elif w == "cfg2b":
            r = cfg2b(a.reps, a.cfg2b_frames, a.placement == "probe", a.cfg2b_header)
        elif w == "cfg3":
            r = cfg3(a.reps, a.cfg3_gib)
        elif w == "cfg3_e2e":
            r = cfg3_e2e(a.cfg3_gib, a.e2e_chunk_mib, min(a.reps, 3))
        elif w == "cfg4":
            r = cfg4(a.reps, a.cfg4_messages, a.placement == "probe")
        elif w == "sync":
            r = sync(max(a.reps, 10))
        elif w == "loopback":
            r = loopback(max(a.reps, 10))
        else:
            r = e2e(a.e2e_gib, a.e2e_chunk_mib, a.e2e_depth)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
