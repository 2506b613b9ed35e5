#!/usr/bin/env python3
"""Times kmws_utf8_validate on one MI355X and prints one JSON line.

The batch: a plain torch.empty arena of 64 KiB FIN text frames, 4 GiB by
default (well past the 256 MiB Infinity Cache), every frame the same 64 KiB of
well-formed text -- in turn all ASCII, mixed 1-3-byte text (a third each by
bytes) and all 3-byte CJK -- and the same batch marked binary (the skip path).
Warm-up, then --calls timed calls each (>= 20), device events, medians.

The bar, from the same process and batch: kmws_unmask_apply with the default
schedule.  The validator reads each byte once and writes nothing, the unmask
reads and writes it, so the ASCII validate must take no longer than that
apply ("ascii_within_unmask_apply"; the exit status is 1 otherwise).  The
mixed and CJK rates and the binary time are recorded, no bar.

Rates: algorithmic bytes (checked payload + 32 B per frame) over the call's
time, and their share of the 8 TB/s HBM peak.  A whole call is timed: the plan,
the three per-frame kernels, the payload pass and the finish.

    python tools/bench_utf8.py [--gib 4] [--calls 20] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME = 65536
PEAK = 8e12


def frame_text(kind: str) -> bytes:
    rng = random.Random(65536)
    out = bytearray()
    if kind == "ascii":
        out += bytes(rng.randint(0x20, 0x7E) for _ in range(FRAME))
    elif kind == "cjk":
        while len(out) + 3 <= FRAME:
            out += chr(rng.randint(0x4E00, 0x9FFF)).encode()
    elif kind == "mixed":  # 6 ASCII + 3 two-byte + 2 three-byte code points per 18 bytes, shuffled
        unit = [1] * 6 + [2] * 3 + [3] * 2
        while len(out) + 18 <= FRAME:
            rng.shuffle(unit)
            for w in unit:
                lo, hi = ((0x20, 0x7E), (0x80, 0x7FF), (0x800, 0xD7FF))[w - 1]
                out += chr(rng.randint(lo, hi)).encode()
    else:
        raise ValueError(kind)
    out += b"." * (FRAME - len(out))
    out.decode("utf-8")  # well-formed, or this raises
    return bytes(out)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch as T
    from kuma_amd import kmws
    if kmws.device_count() < 1:
        print("bench_utf8: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    n = int(a.gib * (1 << 30)) // FRAME
    span = n * FRAME
    arena = T.empty(span, dtype=T.uint8, device="cuda")
    descs = T.empty((n, 2), dtype=T.int64, device="cuda")
    kmws.fill_uniform_descs(descs, FRAME, FRAME, 0x75746638)
    out = T.empty(n, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(kmws.utf8_workspace_size(span, n, 1))
    text_flags = T.full((n,), 0x181, dtype=T.int16, device="cuda")    # FIN | TEXT, mask bit
    binary_flags = T.full((n,), 0x182, dtype=T.int16, device="cuda")  # FIN | BINARY

    def fill(kind):
        pat = T.from_numpy(np.frombuffer(frame_text(kind), dtype=np.uint8).copy()).cuda()
        arena.view(n, FRAME).copy_(pat.unsqueeze(0).expand(n, FRAME))
        T.cuda.synchronize()

    def timed(fn, reps):
        ev = [(T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        T.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}

    def validate(flags):
        kmws.utf8_validate(arena, descs, flags, out, ws, span=span)

    def run_validate(flags, verdict):
        for _ in range(a.warmup):
            validate(flags)
        r = timed(lambda: validate(flags), calls)
        assert ws.status() == 0
        assert bool((out == verdict).all()), "wrong verdicts at the benchmark size"
        return r

    def run_unmask():
        # an even number of applies: the XOR applied twice leaves the text as it was
        kmws.unmask_plan(descs, ws, span)
        for _ in range(2):
            kmws.unmask_apply(arena, descs, ws, span)
        r = timed(lambda: kmws.unmask_apply(arena, descs, ws, span), calls + (calls & 1))
        assert ws.status() == 0
        return r

    res = {"tool": "bench_utf8", "device": T.cuda.get_device_name(0), "frames": n, "frame_bytes": FRAME,
           "span_bytes": span, "calls": calls, "warmup": a.warmup, "allocation": "torch.empty"}
    alg = span + 32 * n
    fill("ascii")
    res["unmask_apply"] = run_unmask()
    for kind in ("ascii", "mixed", "cjk"):
        if kind != "ascii":
            fill(kind)
        r = run_validate(text_flags, kmws.UTF8_OK)
        r["algorithmic_bytes"] = alg
        r["tb_per_s"] = round(alg / (r["median_ms"] * 1e-3) / 1e12, 3)
        r["fraction_of_8tbs_peak"] = round(alg / (r["median_ms"] * 1e-3) / PEAK, 4)
        res["validate_" + kind] = r
    res["validate_binary"] = run_validate(binary_flags, kmws.UTF8_NOT_TEXT)  # the cost of the skip path
    fill("ascii")
    res["unmask_apply_again"] = run_unmask()  # drift over the run
    um = res["unmask_apply"]["median_ms"]
    res["unmask_apply"]["fraction_of_8tbs_peak"] = round((2 * span + 16 * n) / (um * 1e-3) / PEAK, 4)
    res["ascii_over_unmask_apply"] = round(res["validate_ascii"]["median_ms"] / um, 4)
    res["ascii_within_unmask_apply"] = res["validate_ascii"]["median_ms"] <= um
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["ascii_within_unmask_apply"] else 1


if __name__ == "__main__":
    sys.exit(main())
