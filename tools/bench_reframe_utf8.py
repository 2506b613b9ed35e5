#!/usr/bin/env python3
"""Times kmws_unpack_reframe_utf8 against the two calls a relay makes today, on
one MI355X, and prints one JSON line.

A relay of text traffic receives a masked (server-mode) wire, must judge its
text messages (RFC 6455 8.1) and sends the same frames on.  Per shape, payload
kind and outgoing kind, in this one process, whole calls between device events,
alternating a, b, c, a, b, c, ..., the median of --calls (>= 20) of each after
--warmup rounds:

  (a) kmws_unpack_reframe;
  (b) kmws_utf8_validate, payload_masked = 1, on the incoming wire with the
      descriptors and flags the parse wrote;
  (c) kmws_unpack_reframe_utf8 on the same wire.

Three shapes, --gib of payload in the first two (plain torch.empty buffers),
tools/bench_reframe.py's:

  unit   64 KiB FIN frames (65,536 at 4 GiB; dst_cap / n >= 16 KiB: the unit form);
  chunk  4 KiB fragments in 16-fragment messages (1 Mi at 4 GiB; the chunk
         form): the 64 KiB texts cut every 4 KiB, so code points straddle fragments;
  chat   1-300 B frames, 8 Mi of them at 4 GiB, the fragments of one message
         over the same texts.

Four payload kinds (tools/bench_utf8.py's texts): all ASCII, mixed 1-3-byte
text, all 3-byte CJK, and the ASCII bytes marked binary; each with the outgoing
frames unmasked and masked with fresh keys.  Before the timing, the fused
call's dst and wire_off are compared on the device with (a)'s and its verdicts
with (b)'s.

(a) and (b) are the code the fused entry is measured against; it is never
measured against itself.  The bar: (c) < (a) + (b) on the ASCII rows of every
shape ("ascii_fused_below_two_calls"; the exit status is 1 otherwise).  The
mixed and CJK ratios, and binary (c) against (a), are recorded without a bar.

    python tools/bench_reframe_utf8.py [--gib 4] [--calls 20] [--lib PATH] [--commit TEXT] [--out FILE]
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

SEED = 0x72667538


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
        print("bench_reframe_utf8: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    span = int(a.gib * (1 << 30)) // FRAME * FRAME
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

    def run_shape(lens, per_msg):
        """lens: the payload lengths, summing to a multiple of FRAME; per_msg:
        frames per message (0: the whole batch is one message)."""
        n = len(lens)
        P = int(lens.sum())
        rng = np.random.default_rng(SEED + n)
        hl_in = np.where(lens <= 125, 2, np.where(lens <= 65535, 4, 10)) + 4
        W = P + int(hl_in.sum())
        plain_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        in_keys = rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.int64)
        enc_descs = kmws.make_descs(plain_off, lens, in_keys)
        out_keys = T.from_numpy(rng.integers(1, 2**32, size=n, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
        idx = T.arange(n, device=dev)
        head = (idx % per_msg == 0) if per_msg else (idx == 0)
        last = (idx % per_msg == per_msg - 1) if per_msg else (idx == n - 1)
        dense = T.empty(P + 16, dtype=T.uint8, device=dev)
        wire = T.empty(W + 16, dtype=T.uint8, device=dev)
        hdr_off = T.empty(n + 1, dtype=T.int64, device=dev)
        cap_out = W + 16  # a masked outgoing wire is as long as the incoming one
        out_a = T.empty(cap_out, dtype=T.uint8, device=dev)
        out_c = T.empty(cap_out, dtype=T.uint8, device=dev)
        off_a = T.empty(n + 1, dtype=T.int64, device=dev)
        off_c = T.empty(n + 1, dtype=T.int64, device=dev)
        desc_a = T.empty((n, 2), dtype=T.int64, device=dev)
        desc_c = T.empty((n, 2), dtype=T.int64, device=dev)
        fl_a = T.empty(n, dtype=T.int16, device=dev)
        fl_c = T.empty(n, dtype=T.int16, device=dev)
        err = T.empty(n, dtype=T.uint8, device=dev)
        v_b = T.empty(n, dtype=T.uint8, device=dev)
        v_c = T.empty(n, dtype=T.uint8, device=dev)
        ws_e = kmws.Workspace(kmws.copy_workspace_size(n, wire.numel()))
        ws_a = kmws.Workspace(kmws.reframe_workspace_size(n, cap_out))
        ws_b = kmws.Workspace(kmws.utf8_workspace_size(W, n, 1))
        ws_c = kmws.Workspace(kmws.reframe_utf8_workspace_size(n, cap_out, 1))
        res = {"frames": n, "payload_bytes": P, "wire_bytes": W, "frames_per_message": per_msg or n,
               "copy_form": "chunks" if cap_out // n < 16384 else "units"}

        def run_kind(kind, opcode, verdict):
            # the incoming wire: the texts back to back, masked with per-frame keys (setup, not timed)
            pat = T.from_numpy(np.frombuffer(frame_text(kind), dtype=np.uint8).copy()).to(dev)
            dense[:P].view(-1, FRAME).copy_(pat.unsqueeze(0).expand(P // FRAME, FRAME))
            fl_in = (T.where(head, opcode, 0) | T.where(last, 0x80, 0) | kmws.FLAG_MASK).to(T.int16)
            kmws.encode_batch(dense, enc_descs, fl_in, wire, hdr_off, ws_e, check=True)
            row = {}
            for okind, out_mask in (("out_unmasked", 0), ("out_masked", 1)):
                def reframe():
                    kmws.unpack_reframe(wire, hdr_off[:n], kmws.SERVER, desc_a, fl_a, err, 0x0007, out_mask, out_keys,
                                        out_a, off_a, ws_a, wire_len=W)

                def validate():
                    kmws.utf8_validate(wire, desc_a, fl_a, v_b, ws_b, span=W, masked=True)

                def fused():
                    kmws.unpack_reframe_utf8(wire, hdr_off[:n], kmws.SERVER, desc_c, fl_c, err, 0x0007, out_mask,
                                             out_keys, out_c, off_c, v_c, ws_c, wire_len=W)

                for _ in range(a.warmup):
                    reframe(), validate(), fused()
                out_a.fill_(0xEE)
                out_c.fill_(0xEE)
                v_b.fill_(0xEE)
                v_c.fill_(0xEE)
                reframe(), validate(), fused()
                assert ws_a.status() == 0 and ws_b.status() == 0 and ws_c.status() == 0
                assert T.equal(off_c, off_a) and T.equal(desc_c, desc_a) and T.equal(fl_c, fl_a)
                assert T.equal(out_c, out_a), "fused: bytes differ from kmws_unpack_reframe's at the benchmark size"
                assert T.equal(v_c, v_b), "fused: verdicts differ from kmws_utf8_validate's at the benchmark size"
                assert bool((v_c == verdict).all()), "wrong verdicts at the benchmark size"
                r, v, f = timed((reframe, validate, fused), calls)
                assert ws_a.status() == 0 and ws_b.status() == 0 and ws_c.status() == 0
                two = r["median_ms"] + v["median_ms"]
                row[okind] = {"unpack_reframe": r, "validate_masked": v, "fused": f, "two_calls_ms": round(two, 4),
                              "fused_over_two_calls": round(f["median_ms"] / two, 4),
                              "fused_over_unpack_reframe": round(f["median_ms"] / r["median_ms"], 4)}
            return row

        for kind in ("ascii", "mixed", "cjk"):
            res[kind] = run_kind(kind, 1, kmws.UTF8_OK)
        res["binary"] = run_kind("ascii", 2, kmws.UTF8_NOT_TEXT)
        return res

    def chat_lens():
        lens = np.random.default_rng(SEED).integers(1, 301, size=int((8 << 20) * a.gib / 4)).astype(np.int64)
        short = (-int(lens.sum())) % FRAME  # whole texts: the last frames grow by up to 3 bytes each
        k = (short + 2) // 3
        if k:
            lens[-k:] += 3
            lens[-1] -= 3 * k - short
        assert lens.sum() % FRAME == 0 and lens.min() >= 1
        return lens

    shapes = (("unit", np.full(span // FRAME, FRAME, np.int64), 1),
              ("chunk", np.full(span // 4096, 4096, np.int64), FRAME // 4096),
              ("chat", chat_lens(), 0))
    res = {"tool": "bench_reframe_utf8", "device": T.cuda.get_device_name(0), "box": os.uname().nodename,
           "commit": a.commit or commit(), "lib": a.lib or "product", "gib": a.gib, "calls": calls,
           "warmup": a.warmup, "allocation": "torch.empty",
           "order": "unpack_reframe, validate_masked, fused alternating"}
    ok = True
    for name, lens, per_msg in shapes:
        res[name] = run_shape(lens, per_msg)
        T.cuda.empty_cache()
        for okind in ("out_unmasked", "out_masked"):
            ok = ok and res[name]["ascii"][okind]["fused"]["median_ms"] < res[name]["ascii"][okind]["two_calls_ms"]
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
