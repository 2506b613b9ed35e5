#!/usr/bin/env python3
"""What kmws_decoder_set_utf8_check costs on the host path, on one MI355X, in
one process; prints one JSON line.

One RxBatch with an attached pinned ring; a flush's frames lie in the ring and
are unmasked (and, with the check on, validated) there in place.  Two batches:
256 x 64 KiB masked FIN text frames per flush (16 MiB: the launch path either
way), and 64 x 4 KiB (256 KiB: with the check off one job on the resident
worker, with it on a launch -- what leaving the worker costs).  Payloads: all
ASCII; mixed 1-3-byte text; the mixed bytes marked binary (nothing is checked,
so on == off by construction).  Check off and check on alternate, each timed
flush starts from a freshly masked ring (restored untimed), the median of
--flushes (>= 20) after --warmup.  Timed: the deferred feed of the batch (the
header parse and, with the check on, the host half of the message state) plus
kmws_rx_batch_flush, without a frame callback; an untimed first flush with a
callback checks the verdicts.  The baseline is the check-off time of the same
run.  Recorded, no bar.

    python tools/bench_decoder_utf8.py [--flushes 20] [--warmup 3] [--commit TEXT] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_utf8 import frame_text  # noqa: E402  (the same texts)


def commit() -> str:
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def cut_text(text: bytes, n: int) -> bytes:
    """The first n bytes of well-formed text, cut back to a code point boundary and padded."""
    if n >= len(text):
        return text
    e = n
    while e > 0 and (text[e] & 0xC0) == 0x80:
        e -= 1
    out = text[:e] + b"." * (n - e)
    out.decode("utf-8")
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--flushes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--commit", default=None, help="recorded as given (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kuma_amd import kmws

    if kmws.device_count() < 1:
        print("no gfx950 device", file=sys.stderr)
        return 2
    rows = []
    for nframes, flen in ((256, 65536), (64, 4096)):
        for kind in ("ascii", "mixed", "binary"):
            body = cut_text(frame_text("mixed" if kind == "binary" else kind), flen)
            opcode = kmws.OP_BINARY if kind == "binary" else kmws.OP_TEXT
            rng = np.random.default_rng(flen + len(kind))
            wire = bytearray()
            p = np.frombuffer(body, dtype=np.uint8)
            for _ in range(nframes):
                key = bytes(int(x) for x in rng.integers(0, 256, 4))
                hdr = kmws.encode_frame_header(kmws.Header(fin=1, opcode=opcode, mask=1, maskey=key, length=flen))
                k = np.frombuffer(key * (flen // 4), dtype=np.uint8)
                wire += hdr + (p ^ k).tobytes()
            masked = torch.frombuffer(wire, dtype=torch.uint8).clone()
            ring = torch.zeros(len(wire), dtype=torch.uint8).pin_memory()
            batch = kmws.RxBatch()
            batch.attach_ring(ring)
            handlers = {}
            for on in (False, True):
                h = kmws.WSHandler(kmws.SERVER)
                h.setUtf8Check(on)
                handlers[on] = h

            def one(on, cb=None):
                h = handlers[on]
                h.setFrameCallback(cb)
                ring.copy_(masked)
                t0 = time.perf_counter()
                rc = h.handleDataDeferredPtr(batch, ring.data_ptr(), len(wire))
                t1 = time.perf_counter()
                n = batch.flush()
                t2 = time.perf_counter()
                assert rc == kmws.WS_NOERR and n == nframes, (rc, n)
                return (t2 - t0) * 1e6, (t2 - t1) * 1e6

            # untimed: the verdicts and the bytes, once per setting
            for on in (False, True):
                seen = []
                one(on, lambda hd, pl: seen.append((hd.utf8, pl == body)) and None)
                want = kmws.UTF8_OK if (on and kind != "binary") else 0
                assert seen == [(want, True)] * nframes, (kind, on, seen[:3])
            times = {False: [], True: []}
            for i in range(a.warmup + a.flushes):
                for on in (False, True):
                    t = one(on)
                    if i >= a.warmup:
                        times[on].append(t)
            med = {on: [statistics.median(x[j] for x in times[on]) for j in (0, 1)] for on in (False, True)}
            rows.append({"frames": nframes, "frame_bytes": flen, "payload": kind,
                         "off_us": round(med[False][0], 1), "on_us": round(med[True][0], 1),
                         "on_over_off": round(med[True][0] / med[False][0], 3),
                         "flush_off_us": round(med[False][1], 1), "flush_on_us": round(med[True][1], 1),
                         "flush_on_over_off": round(med[True][1] / med[False][1], 3)})
            del batch
    res = {"bench": "decoder_utf8", "commit": a.commit or commit(), "device": torch.cuda.get_device_name(0),
           "flushes": a.flushes, "warmup": a.warmup,
           "timed": "deferred feed + kmws_rx_batch_flush, pinned ring, no callback; *_us medians; flush_*: the flush alone",
           "rows": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
