#!/usr/bin/env python3
"""kuma's call pattern with kmws_decoder_set_utf8_check on and off, on one and
on eight loop threads, on one MI355X; prints one JSON line.

Each thread owns an RxBatch, a pinned ring and a handler, and per flush feeds
one 64 KiB read -- 16 masked FIN frames of 4 KiB, in place in its ring -- and
flushes it: the job the resident worker exists for.  Texts: all ASCII; mixed
1-3-byte (tools/bench_utf8.py frame_text); the mixed bytes marked binary
(nothing is checked).  Timed per flush: kmws_decoder_feed_deferred +
kmws_rx_batch_flush, without a frame callback (the ctypes calls release the
GIL); the ring is restored to the masked wire untimed before each (a plain
memmove: a torch copy of this size starts a thread team per calling thread).
The interpreter's switch interval is set to 1 us so that a thread coming back
from a call is not kept waiting for the lock by another one's bookkeeping.  The
threads of a row start together; a row reports each thread's median flush time
and the aggregate rate sum over threads of (wire bytes per flush / median).
Uses only binding calls older than the resident worker's check, so the same
file measures an earlier checkout: copy it into that checkout's tools/.

    python tools/bench_resident_utf8.py [--flushes 200] [--warmup 20] [--commit TEXT] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_utf8 import frame_text  # noqa: E402

NFRAMES, FLEN = 16, 4096


def commit() -> str:
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def cut_text(text: bytes, n: int) -> bytes:
    """The first n bytes of well-formed text, cut back to a code point boundary and padded."""
    e = n
    while e > 0 and (text[e] & 0xC0) == 0x80:
        e -= 1
    out = text[:e] + b"." * (n - e)
    out.decode("utf-8")
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--flushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--commit", default=None, help="recorded as given (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes
    import numpy as np
    import torch
    from kuma_amd import kmws

    torch.set_num_threads(1)
    sys.setswitchinterval(1e-6)

    if kmws.device_count() < 1:
        print("no gfx950 device", file=sys.stderr)
        return 2

    def wire_of(kind, seed):
        body = cut_text(frame_text("mixed" if kind == "binary" else kind), FLEN)
        opcode = kmws.OP_BINARY if kind == "binary" else kmws.OP_TEXT
        rng = np.random.default_rng(seed)
        p = np.frombuffer(body, dtype=np.uint8)
        wire = bytearray()
        for _ in range(NFRAMES):
            key = bytes(int(x) for x in rng.integers(0, 256, 4))
            hdr = kmws.encode_frame_header(kmws.Header(fin=1, opcode=opcode, mask=1, maskey=key, length=FLEN))
            wire += hdr + (p ^ np.frombuffer(key * (FLEN // 4), dtype=np.uint8)).tobytes()
        return body, wire

    def worker(kind, on, tid, start, out):
        try:
            body, wire = wire_of(kind, 100 * tid + len(kind))
            masked = torch.frombuffer(wire, dtype=torch.uint8).clone()
            ring = torch.zeros(len(wire), dtype=torch.uint8).pin_memory()
            batch = kmws.RxBatch()
            batch.attach_ring(ring)
            h = kmws.WSHandler(kmws.SERVER)
            h.setUtf8Check(on)
            feed, flush, ptr, n = h.handleDataDeferredPtr, batch.flush, ring.data_ptr(), len(wire)
            restore, src = ctypes.memmove, masked.data_ptr()
            # untimed: the verdicts and the bytes, once
            seen = []
            h.setFrameCallback(lambda hd, pl: seen.append((hd.utf8, pl == body)) and None)
            ring.copy_(masked)
            assert feed(batch, ptr, n) == kmws.WS_NOERR and flush() == NFRAMES
            want = kmws.UTF8_OK if (on and kind != "binary") else 0
            assert seen == [(want, True)] * NFRAMES, (kind, on, seen[:3])
            h.setFrameCallback(None)
            times = []
            start.wait()
            for i in range(a.warmup + a.flushes):
                restore(ptr, src, n)
                t0 = time.perf_counter()
                rc = feed(batch, ptr, n)
                k = flush()
                t1 = time.perf_counter()
                if rc != kmws.WS_NOERR or k != NFRAMES:
                    raise RuntimeError(f"feed {rc}, flush {k}")
                if i >= a.warmup:
                    times.append((t1 - t0) * 1e6)
            out[tid] = (statistics.median(times), n)
        except BaseException as e:
            out[tid] = e
            try:
                start.abort()
            except Exception:
                pass

    rows = []
    # every check-off row before the first check-on one: from its first checked
    # job on a process's grid is the validating instantiation, and a process
    # that never turns the check on is what the check-off rows stand for
    for on in (False, True):
        for nthreads in (1, 8):
            for kind in ("ascii", "mixed", "binary"):
                out = [None] * nthreads
                start = threading.Barrier(nthreads)
                ths = [threading.Thread(target=worker, args=(kind, on, t, start, out)) for t in range(nthreads)]
                for th in ths:
                    th.start()
                for th in ths:
                    th.join()
                for r in out:
                    if isinstance(r, BaseException):
                        raise r
                meds = [r[0] for r in out]
                agg = sum(r[1] / (r[0] * 1e-6) for r in out) / 2**30
                rows.append({"threads": nthreads, "payload": kind, "check": int(on),
                             "median_us": round(statistics.median(meds), 2),
                             "thread_median_us": [round(m, 2) for m in meds], "agg_gib_s": round(agg, 3)})
    res = {"bench": "resident_utf8", "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0),
           "flushes": a.flushes, "warmup": a.warmup, "frames": NFRAMES, "frame_bytes": FLEN,
           "timed": "kmws_decoder_feed_deferred + kmws_rx_batch_flush of one 64 KiB read in a pinned ring, no callback; "
                    "agg_gib_s = sum over threads of wire bytes / median flush time",
           "rows": rows}
    if hasattr(kmws, "resident_utf8"):
        res["resident_utf8"] = kmws.resident_utf8()
    res["resident_jobs"] = kmws.resident_info()["jobs"]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
