#!/usr/bin/env python3
"""Times kmws_unpack_reframe against the two calls it replaces, on one MI355X,
and prints one JSON line.

A relay receives a masked (server-mode) wire and sends the same frames on.  Per
shape, in this one process, whole calls between device events, alternating a, b,
c, a, b, c, ..., the median of --calls (>= 20) of each after --warmup rounds:

  (a) kmws_unpack_gather: parse, unmask, payloads dense;
  (b) kmws_encode_batch on the gather's output (descriptors from dst_off);
  (c) kmws_unpack_reframe on the same wire.

Three shapes, --gib of payload in the first two (plain torch.empty buffers):

  unit   64 KiB FIN binary frames (65,536 at 4 GiB; dst_cap / n >= 16 KiB: the unit form);
  chunk  4 KiB fragments (1 Mi at 4 GiB; the chunk form);
  chat   1-300 B frames, 8 Mi of them at 4 GiB (the 8 M-frame row of the README,
         scaled with --gib).

Each with the outgoing frames unmasked and masked with fresh keys.  Before the
timing, one fused call's output is compared on the device with what (a) + (b)
wrote, and 64 sampled frames with the oracle (unmask + encode on the host).

The bar: (c) < (a) + (b) on every shape and outgoing kind ("fused_below_two_calls";
the exit status is 1 otherwise).  The ratio to (b) alone, which moves the same
bytes, is recorded without a bar.

    python tools/bench_reframe.py [--gib 4] [--calls 20] [--lib PATH] [--commit TEXT] [--out FILE]
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

SEED = 0x7265667261


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
    from oracle import oracle as orc
    if a.lib:
        kmws.lib()  # torch's HIP runtime first, as the product library has it
        kmws._lib = kmws.bind(ctypes.CDLL(os.path.abspath(a.lib)))
    if kmws.device_count() < 1:
        print("bench_reframe: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    span = int(a.gib * (1 << 30))
    dev = "cuda"

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

    def run_shape(name, lens):
        n = len(lens)
        P = int(lens.sum())
        rng = np.random.default_rng(SEED + n)
        hl_in = np.where(lens <= 125, 2, np.where(lens <= 65535, 4, 10)) + 4
        W = P + int(hl_in.sum())
        # the incoming wire: synthetic payloads, masked with per-frame keys (setup, not timed)
        dense = T.empty(P + 16, dtype=T.uint8, device=dev)
        kmws.fill_synthetic(dense, SEED)
        plain_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        in_keys = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.int64)
        wire = T.empty(W + 16, dtype=T.uint8, device=dev)
        hdr_off = T.empty(n + 1, dtype=T.int64, device=dev)
        fl_in = T.full((n,), 0x82 | kmws.FLAG_MASK, dtype=T.int16, device=dev)
        ws0 = kmws.Workspace(kmws.copy_workspace_size(n, wire.numel()))
        kmws.encode_batch(dense, kmws.make_descs(plain_off, lens, in_keys), fl_in, wire, hdr_off, ws0, check=True)
        del ws0
        out_keys_np = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
        out_keys = T.from_numpy(out_keys_np.view(np.int32)).to(dev)
        out_desc = T.empty((n, 2), dtype=T.int64, device=dev)
        out_flags = T.empty(n, dtype=T.int16, device=dev)
        out_err = T.empty(n, dtype=T.uint8, device=dev)
        dst_off = T.empty(n + 1, dtype=T.int64, device=dev)
        cap_out = W + 16  # a masked outgoing wire is as long as the incoming one
        out_two = T.empty(cap_out, dtype=T.uint8, device=dev)
        out_fused = T.empty(cap_out, dtype=T.uint8, device=dev)
        off_two = T.empty(n + 1, dtype=T.int64, device=dev)
        off_fused = T.empty(n + 1, dtype=T.int64, device=dev)
        ws_g = kmws.Workspace(kmws.copy_workspace_size(n, dense.numel()))
        ws_e = kmws.Workspace(kmws.copy_workspace_size(n, cap_out))
        ws_f = kmws.Workspace(kmws.reframe_workspace_size(n, cap_out))
        form = "chunks" if cap_out // n < 16384 else "units"
        res = {"frames": n, "payload_bytes": P, "wire_bytes": W, "copy_form": form}
        enc_desc = T.empty((n, 2), dtype=T.int64, device=dev)
        lens_d = T.from_numpy(lens).to(dev)

        def gather():
            kmws.unpack_gather(wire, hdr_off[:n], kmws.SERVER, out_desc, out_flags, out_err, dense, dst_off, ws_g,
                               wire_len=W)

        for kind, out_mask in (("out_unmasked", 0), ("out_masked", 1)):
            fl_out = T.full((n,), 0x82 | (kmws.FLAG_MASK if out_mask else 0), dtype=T.int16, device=dev)
            gather()
            # the encode's descriptors: the gather's offsets, the outgoing keys (setup, not timed)
            enc_desc[:, 0] = dst_off[:n]
            enc_desc[:, 1] = lens_d | ((out_keys.to(T.int64) & 0xFFFFFFFF) << 32 if out_mask else 0)

            def encode():
                kmws.encode_batch(dense, enc_desc, fl_out, out_two, off_two, ws_e)

            def fused():
                kmws.unpack_reframe(wire, hdr_off[:n], kmws.SERVER, out_desc, out_flags, out_err, 0x0007, out_mask,
                                    out_keys, out_fused, off_fused, ws_f, wire_len=W)

            for _ in range(a.warmup):
                gather(), encode(), fused()
            out_two.fill_(0xEE)
            out_fused.fill_(0xEE)
            gather(), encode(), fused()
            assert ws_g.status() == 0 and ws_e.status() == 0 and ws_f.status() == 0
            total = int(off_two[n])
            assert total == P + int((hl_in - (0 if out_mask else 4)).sum())
            assert T.equal(off_fused, off_two), "fused: wrong offsets at the benchmark size"
            assert T.equal(out_fused[:total], out_two[:total]), "fused: bytes differ from gather + encode"
            assert bool((out_fused[total:] == 0xEE).all())
            offs_h = off_fused.cpu().numpy()
            for f in np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, size=62)])):  # the oracle, sampled
                f = int(f)
                h = int(hdr_off[f])
                raw = wire[h + int(hl_in[f]):h + int(hl_in[f]) + int(lens[f])].cpu().numpy().copy()
                d = np.zeros(1, dtype=orc.DESC_DTYPE)
                d["len"], d["key"] = int(lens[f]), int(in_keys[f])
                orc.unmask_batch(raw, d)
                want, _ = orc.encode_batch(np.concatenate([raw, np.zeros(16, np.uint8)]), np.zeros(1, np.uint64),
                                           lens[f:f + 1], np.array([0x82 | (0x100 if out_mask else 0)], np.uint32),
                                           out_keys_np[f:f + 1] if out_mask else np.zeros(1, np.uint32))
                got = out_fused[int(offs_h[f]):int(offs_h[f + 1])].cpu().numpy()
                assert np.array_equal(got, want), f"fused: frame {f} differs from the oracle"
            g, e, f3 = timed((gather, encode, fused), calls)
            assert ws_g.status() == 0 and ws_e.status() == 0 and ws_f.status() == 0
            two = g["median_ms"] + e["median_ms"]
            res[kind] = {"unpack_gather": g, "encode_batch": e, "fused": f3, "two_calls_ms": round(two, 4),
                         "fused_over_two_calls": round(f3["median_ms"] / two, 4),
                         "fused_over_encode_batch": round(f3["median_ms"] / e["median_ms"], 4),
                         "fused_frac_of_8TBps": round((W + total) / (f3["median_ms"] * 1e-3) / 8e12, 4),
                         "out_bytes": total}
        return res

    shapes = (("unit", np.full(span // 65536, 65536, np.int64)),
              ("chunk", np.full(span // 4096, 4096, np.int64)),
              ("chat", np.random.default_rng(SEED).integers(1, 301, size=int((8 << 20) * a.gib / 4)).astype(np.int64)))
    res = {"tool": "bench_reframe", "device": T.cuda.get_device_name(0), "box": os.uname().nodename,
           "commit": a.commit or commit(), "lib": a.lib or "product", "gib": a.gib, "calls": calls,
           "warmup": a.warmup, "allocation": "torch.empty", "order": "unpack_gather, encode_batch, fused alternating"}
    ok = True
    for name, lens in shapes:
        res[name] = run_shape(name, lens)
        T.cuda.empty_cache()
        for kind in ("out_unmasked", "out_masked"):
            ok = ok and res[name][kind]["fused"]["median_ms"] < res[name][kind]["two_calls_ms"]
    res["fused_below_two_calls"] = ok
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
