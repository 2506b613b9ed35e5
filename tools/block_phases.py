#!/usr/bin/env python3
"""Where an apply block of the headline batch spends its time.

Loads the diagnostic build of the library by path (KMWS_DIAG_PHASE_STAMPS
through kuma_amd/build.py `defines`; never kmws.lib(), never a product
variant), runs the headline shape -- 64 KiB frames in an aligned arena, the
default schedule -- and reads the six s_memtime stamps one block in 1024
kept: entry, index math done, payload loads issued, metadata arrived, first
payload word arrived, last store issued (with staged loads, kUnmaskDepth below
4: the up-front loads issued, and the store phase holds the later loads and
the waits for the later words).  Prints the median share of each
phase of the block's entry-to-last-store time, in shader cycles.  Stamping
costs about a tenth of the wave's cycles, so this is a record of shares.

usage: python3 tools/block_phases.py [--build] [--lib PATH] [--gib 64] [--applies 5]
  --build only builds the diagnostic library (no GPU needed) and prints its path."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIAG_LIB = os.path.join(ROOT, "build_variants", "libkmws_gpu_phases.so")
PHASES = ["index math", "issue payload loads", "wait for metadata", "wait for first payload word",
          "xor and issue stores"]
EVERY, STAMPS = 1024, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--lib", default=DIAG_LIB)
    ap.add_argument("--gib", type=int, default=64)
    ap.add_argument("--applies", type=int, default=5)
    a = ap.parse_args()
    if a.build:
        from kuma_amd import build as kb
        print(kb.build(out=a.lib, defines=("KMWS_DIAG_PHASE_STAMPS=1",)))
        return
    import numpy as np
    import torch
    from kuma_amd import kmws
    L = kmws.bind(C.CDLL(a.lib))
    L.kmws_diag_set_stamps.restype = C.c_int
    L.kmws_diag_set_stamps.argtypes = [C.c_void_p, C.c_uint32]
    frame = 65536
    span = a.gib << 30
    n = span // frame
    base = torch.empty(span, dtype=torch.uint8, device="cuda")
    descs = torch.empty((n, 2), dtype=torch.int64, device="cuda")
    assert L.kmws_fill_synthetic(base.data_ptr(), span, 0x6B756D61, None) == 0
    assert L.kmws_fill_uniform_descs(descs.data_ptr(), n, frame, frame, 99, None) == 0
    ws = torch.empty(L.kmws_unmask_workspace_size(span), dtype=torch.uint8, device="cuda")
    slots = (span // 16384 + EVERY - 1) // EVERY
    stamps = torch.zeros((slots, STAMPS), dtype=torch.int64, device="cuda")
    assert L.kmws_unmask_plan(span, descs.data_ptr(), n, ws.data_ptr(), ws.numel(), None) == 0
    assert L.kmws_diag_set_stamps(None, 0) == 0
    for _ in range(2):  # warm up unstamped
        assert L.kmws_unmask_apply(base.data_ptr(), span, descs.data_ptr(), n, ws.data_ptr(), ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert L.kmws_diag_set_stamps(stamps.data_ptr(), slots) == 0
    rows = []
    for _ in range(a.applies):
        stamps.zero_()
        assert L.kmws_unmask_apply(base.data_ptr(), span, descs.data_ptr(), n, ws.data_ptr(), ws.numel(), None) == 0
        torch.cuda.synchronize()
        rows.append(stamps.cpu().numpy().astype(np.int64))
    assert L.kmws_diag_set_stamps(None, 0) == 0
    t = np.concatenate(rows)
    t = t[t[:, STAMPS - 1] != 0]
    d = np.diff(t, axis=1).astype(np.float64)
    keep = (d >= 0).all(axis=1)
    d = d[keep]
    total = d.sum(axis=1)
    out = {"lib": os.path.relpath(a.lib, ROOT), "gib": a.gib, "applies": a.applies, "stamped_blocks": int(len(d)),
           "dropped_non_monotonic": int((~keep).sum()),
           "block_cycles": {"median": float(np.median(total)), "p10": float(np.percentile(total, 10)),
                            "p90": float(np.percentile(total, 90))},
           "phases": {}}
    for i, name in enumerate(PHASES):
        out["phases"][name] = {"median_cycles": float(np.median(d[:, i])),
                               "median_share": round(float(np.median(d[:, i] / total)), 4),
                               "p90_cycles": float(np.percentile(d[:, i], 90))}
    print(json.dumps(out, indent=1))
    for name, p in out["phases"].items():
        print(f"{name:30s} median {p['median_cycles']:9.0f} cycles  share {100 * p['median_share']:5.1f} %", file=sys.stderr)


if __name__ == "__main__":
    main()
