#!/usr/bin/env python3
"""Times kmws_unmask_utf8_batch against the two calls it replaces, on one
MI355X, and prints one JSON line.

The batch of tools/bench_utf8.py: a plain torch.empty arena of 65,536 x 64 KiB
FIN text frames (4 GiB), every frame the same 64 KiB of well-formed text -- in
turn all ASCII, mixed 1-3-byte text, all 3-byte CJK -- masked with per-frame
keys, and the ASCII bytes marked binary.  Per kind, in this one process, whole
calls between device events, the median of --calls (>= 20) after --warmup:

  (a) kmws_unmask_batch alone (plan + apply; an even number of calls, so the
      arena ends masked again);
  (b) kmws_utf8_validate(payload_masked = 1) alone, on the masked arena;
  (c) kmws_unmask_utf8_batch.  Every timed call starts from masked bytes: an
      untimed kmws_unmask_apply between the calls masks the arena again (the
      XOR is its own inverse).

(a) and (b) are the code the fused entry is measured against; it is never
measured against itself.  The bar: on the ASCII batch (c) < (a) + (b)
("ascii_fused_below_two_calls"; the exit status is 1 otherwise).  The mixed and
CJK ratios and binary (c) against (a) are recorded, no bar.

    python tools/bench_unmask_utf8.py [--gib 4] [--calls 20] [--lib PATH] [--commit TEXT] [--out FILE]

--lib: a variant build of the library (kuma_amd/build.py `out` + `srcdir` or
`defines`) instead of the product library.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_utf8 import FRAME, frame_text  # noqa: E402  (the same texts)


def commit() -> str:
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return "unknown"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--commit", default=None, help="recorded as given (default: git rev-parse --short HEAD)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch as T
    from kuma_amd import kmws
    if a.lib:
        kmws.lib()  # torch's HIP runtime first, as the product library has it
        kmws._lib = kmws.bind(ctypes.CDLL(os.path.abspath(a.lib)))
    if kmws.device_count() < 1:
        print("bench_unmask_utf8: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    calls += calls & 1
    n = int(a.gib * (1 << 30)) // FRAME
    span = n * FRAME
    arena = T.empty(span, dtype=T.uint8, device="cuda")
    descs = T.empty((n, 2), dtype=T.int64, device="cuda")
    kmws.fill_uniform_descs(descs, FRAME, FRAME, 0x75746638)
    out = T.empty(n, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.unmask_utf8_workspace_size(span, n, 1))  # holds the validator's and the unmask's too
    ws_mask = kmws.Workspace(kmws.unmask_workspace_size(span))        # the plan of the untimed re-masking apply
    kmws.unmask_plan(descs, ws_mask, span)
    text_flags = T.full((n,), 0x181, dtype=T.int16, device="cuda")    # FIN | TEXT, mask bit
    binary_flags = T.full((n,), 0x182, dtype=T.int16, device="cuda")  # FIN | BINARY

    def remask():
        kmws.unmask_apply(arena, descs, ws_mask, span)

    def fill_masked(kind):
        pat = T.from_numpy(np.frombuffer(frame_text(kind), dtype=np.uint8).copy()).cuda()
        arena.view(n, FRAME).copy_(pat.unsqueeze(0).expand(n, FRAME))
        remask()
        T.cuda.synchronize()
        return pat

    def timed(fn, reps, between=None):
        ev = [(T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
            if between:
                between()
        T.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    def run_kind(kind, flags, verdict):
        pat = fill_masked(kind)
        r = {}
        unmask = lambda: kmws.unmask_batch(arena, descs, ws, span)
        for _ in range(a.warmup + (a.warmup & 1)):
            unmask()
        r["unmask_batch"] = timed(unmask, calls)  # even: masked again
        assert ws.status() == 0
        validate = lambda: kmws.utf8_validate(arena, descs, flags, out, ws, span=span, masked=True)
        for _ in range(a.warmup):
            validate()
        out.fill_(0xEE)
        r["validate_masked"] = timed(validate, calls)
        assert ws.status() == 0 and bool((out == verdict).all()), "validate: wrong verdicts at the benchmark size"
        fused = lambda: kmws.unmask_utf8(arena, descs, flags, out, ws, span=span)
        for _ in range(a.warmup):
            fused()
            remask()
        out.fill_(0xEE)
        r["fused"] = timed(fused, calls, between=remask)
        assert ws.status() == 0 and bool((out == verdict).all()), "fused: wrong verdicts at the benchmark size"
        fused()  # and the bytes: the arena is plain after one more call
        assert bool((arena.view(n, FRAME) == pat.unsqueeze(0)).all()), "fused: wrong bytes at the benchmark size"
        two = r["unmask_batch"]["median_ms"] + r["validate_masked"]["median_ms"]
        r["two_calls_ms"] = round(two, 4)
        r["fused_over_two_calls"] = round(r["fused"]["median_ms"] / two, 4)
        r["fused_over_unmask_batch"] = round(r["fused"]["median_ms"] / r["unmask_batch"]["median_ms"], 4)
        return r

    res = {"tool": "bench_unmask_utf8", "device": T.cuda.get_device_name(0), "box": os.uname().nodename,
           "commit": a.commit or commit(), "lib": a.lib or "product", "frames": n, "frame_bytes": FRAME, "span_bytes": span,
           "calls": calls, "warmup": a.warmup, "allocation": "torch.empty",
           "fused_calls_start_from": "masked bytes (an untimed kmws_unmask_apply between the timed calls)"}
    for kind in ("ascii", "mixed", "cjk"):
        res[kind] = run_kind(kind, text_flags, kmws.UTF8_OK)
    res["binary"] = run_kind("ascii", binary_flags, kmws.UTF8_NOT_TEXT)
    res["ascii_fused_below_two_calls"] = res["ascii"]["fused"]["median_ms"] < res["ascii"]["two_calls_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["ascii_fused_below_two_calls"] else 1


if __name__ == "__main__":
    sys.exit(main())
