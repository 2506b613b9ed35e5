#!/usr/bin/env python3
"""Times kmws_gather_unmask_utf8 against the two calls it replaces, on one
MI355X, and prints one JSON line.

Two batch shapes on plain torch.empty buffers (--gib of source each, and as
much of dst), the payloads packed back to back in src and masked with per-frame
keys:

  unit   65,536 x 64 KiB FIN text frames (dst_cap / n >= 16 KiB: copy_kernel);
  chunk  1 Mi x 4 KiB fragments in 16-fragment messages (the chunk form): the
         same 64 KiB texts cut every 4 KiB, so code points straddle fragments.

Four payload kinds (tools/bench_utf8.py's texts): all ASCII, mixed 1-3-byte
text, all 3-byte CJK, and the ASCII bytes marked binary.  Per shape and kind, in
this one process, whole calls between device events, alternating a, b, c, a, b,
c, ..., the median of --calls (>= 20) of each after --warmup rounds:

  (a) kmws_gather_unmask;
  (b) kmws_utf8_validate on the dense output, plain (descriptors from dst_off);
  (c) kmws_gather_unmask_utf8.

(a) and (b) are the code the fused entry is measured against; it is never
measured against itself.  The bar: on the ASCII batch of both shapes (c) < (a)
+ (b) ("ascii_fused_below_two_calls"; the exit status is 1 otherwise).  The
mixed and CJK ratios and binary (c) against (a) are recorded, no bar.

    python tools/bench_gather_utf8.py [--gib 4] [--calls 20] [--lib PATH] [--commit TEXT] [--out FILE]

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

SHAPES = (("unit", FRAME, 1), ("chunk", 4096, FRAME // 4096))  # name, frame bytes, frames per message


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
        print("bench_gather_utf8: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    span = int(a.gib * (1 << 30)) // FRAME * FRAME
    src = T.empty(span, dtype=T.uint8, device="cuda")
    dst = T.empty(span, dtype=T.uint8, device="cuda")

    def timed(fns, reps):
        ev = [[(T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
        for row in ev:
            for fn, (e0, e1) in zip(fns, row):
                e0.record()
                fn()
                e1.record()
        T.cuda.synchronize()
        res = []
        for k in range(len(fns)):
            ms = sorted(row[k][0].elapsed_time(row[k][1]) for row in ev)
            res.append({"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4),
                        "max_ms": round(ms[-1], 4)})
        return res

    def run_shape(frame, per_msg):
        n = span // frame
        assert (span // n >= 16384) == (per_msg == 1)  # the copy form the shape is meant to take
        descs = T.empty((n, 2), dtype=T.int64, device="cuda")
        kmws.fill_uniform_descs(descs, frame, frame, 0x75746638)
        dense = descs.clone()  # the dense output's descriptors: the same offsets (the source is packed too)
        off = T.empty(n + 1, dtype=T.int64, device="cuda")
        out = T.empty(n, dtype=T.uint8, device="cuda")
        ws_copy = kmws.Workspace(kmws.copy_workspace_size(n, span))
        ws_val = kmws.Workspace(kmws.utf8_workspace_size(span, n, 1))
        ws_fused = kmws.Workspace(kmws.gather_utf8_workspace_size(n, span, 1))
        ws_mask = kmws.Workspace(kmws.unmask_workspace_size(span))  # the plan of the untimed masking apply
        kmws.unmask_plan(descs, ws_mask, span)
        pos = T.arange(n, device="cuda") % per_msg
        res = {"frames": n, "frame_bytes": frame, "frames_per_message": per_msg}

        def run_kind(kind, opcode, verdict):
            pat = T.from_numpy(np.frombuffer(frame_text(kind), dtype=np.uint8).copy()).cuda()
            src.view(-1, FRAME).copy_(pat.unsqueeze(0).expand(span // FRAME, FRAME))
            kmws.unmask_apply(src, descs, ws_mask, span)  # masked with the descriptors' keys
            fin = T.where(pos == per_msg - 1, 0x80, 0)
            flags = (T.where(pos == 0, opcode, 0) | fin | 0x100).to(T.int16)
            gather = lambda: kmws.gather_unmask(src, descs, dst, off, ws_copy)
            validate = lambda: kmws.utf8_validate(dst, dense, flags, out, ws_val, span=span, masked=False)
            fused = lambda: kmws.gather_unmask_utf8(src, descs, flags, dst, off, out, ws_fused)
            for _ in range(a.warmup):
                gather(), validate(), fused()
            dst.fill_(0xEE)
            out.fill_(0xEE)
            fused()
            assert ws_fused.status() == 0 and bool((out == verdict).all()), "fused: wrong verdicts at the benchmark size"
            assert bool((dst.view(-1, FRAME) == pat.unsqueeze(0)).all()), "fused: wrong bytes at the benchmark size"
            g, v, f = timed((gather, validate, fused), calls)
            assert ws_copy.status() == 0 and ws_val.status() == 0 and ws_fused.status() == 0
            assert bool((out == verdict).all())
            two = g["median_ms"] + v["median_ms"]
            return {"gather_unmask": g, "validate_plain": v, "fused": f, "two_calls_ms": round(two, 4),
                    "fused_over_two_calls": round(f["median_ms"] / two, 4),
                    "fused_over_gather_unmask": round(f["median_ms"] / g["median_ms"], 4)}

        for kind in ("ascii", "mixed", "cjk"):
            res[kind] = run_kind(kind, 1, kmws.UTF8_OK)
        res["binary"] = run_kind("ascii", 2, kmws.UTF8_NOT_TEXT)
        return res

    res = {"tool": "bench_gather_utf8", "device": T.cuda.get_device_name(0), "box": os.uname().nodename,
           "commit": a.commit or commit(), "lib": a.lib or "product", "span_bytes": span, "calls": calls,
           "warmup": a.warmup, "allocation": "torch.empty", "order": "gather, validate, fused alternating"}
    ok = True
    for name, frame, per_msg in SHAPES:
        res[name] = run_shape(frame, per_msg)
        ok = ok and res[name]["ascii"]["fused"]["median_ms"] < res[name]["ascii"]["two_calls_ms"]
    res["ascii_fused_below_two_calls"] = ok
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
