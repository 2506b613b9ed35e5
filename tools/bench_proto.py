#!/usr/bin/env python3
"""Times kmws_proto_check on one MI355X and prints one JSON line.

The batch: 8,388,608 chat-sized frames (1-300 B payloads, masked, the relay
row's shape) of 65,536 streams, 128 frames each, laid out as a server-mode wire
on the device: seven of eight messages are one FIN BINARY frame, the eighth is
a BINARY head and a CONTINUE.  kmws_unpack_headers parses it once; its
out_desc / out_flags / out_err are what the timed calls get.

Timed, whole calls, alternating in one process, device events, medians of
--calls (>= 20) each:
  kmws_proto_check    (three launches, 1 B + 1 B of elements per frame);
  kmws_utf8_validate  on the same batch -- every message is binary, so this is
                      the cost of the project's other per-frame segmented scan
                      (seven launches, 12 B of elements per frame);
  kmws_unpack_headers (the per-frame front both follow).
The bar: the proto check takes no longer than that validate call
("proto_within_utf8_binary"; the exit status is 1 otherwise).

Then the same shape once more with every stream's last frame (every 128th) a
CLOSE carrying a 123-byte reason of 3-byte code points, which the owning lane
walks serially: recorded, no bar.

    python tools/bench_proto.py [--frames 8388608] [--streams 65536] [--calls 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8388608)
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch as T
    from kuma_amd import kmws
    if kmws.device_count() < 1:
        print("bench_proto: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    n, ns = a.frames, a.streams
    per = n // ns
    assert per * ns == n and per % 8 == 0, "whole streams of whole 8-frame groups"
    dev = "cuda"

    def build(with_close):
        """-> (wire, wire_len, hdr_off): the wire on the device."""
        g = T.Generator(device=dev)
        g.manual_seed(6455)
        lens = T.randint(1, 301, (n,), device=dev, generator=g, dtype=T.int64)
        pos = T.arange(n, device=dev, dtype=T.int64) % per
        b0 = T.full((n,), 0x82, dtype=T.int64, device=dev)
        b0[pos % 8 == 0] = 0x02  # a BINARY head ...
        b0[pos % 8 == 1] = 0x80  # ... and its CONTINUE
        last = pos == per - 1
        if with_close:
            lens[last] = 125
            b0[last] = 0x88
        hlen = T.where(lens < 126, 6, 8)
        size = hlen + lens
        hdr_off = T.cumsum(size, 0) - size
        wire_len = int(size.sum().item())
        wire = T.full(((wire_len + 31) // 16 * 16,), 0x61, dtype=T.uint8, device=dev)
        wire[hdr_off] = b0.to(T.uint8)
        wire[hdr_off + 1] = T.where(lens < 126, 0x80 | lens, T.full_like(lens, 0x80 | 126)).to(T.uint8)
        big = lens >= 126
        wire[hdr_off[big] + 2] = (lens[big] >> 8).to(T.uint8)
        wire[hdr_off[big] + 3] = (lens[big] & 0xFF).to(T.uint8)
        # the mask keys: whatever the fill left (0x61616161) -- the payloads are not looked at ...
        if with_close:
            # ... but the CLOSE bodies are: key 0, so the bytes written are the masked bytes
            body = bytes([0x03, 0xE8]) + "€".encode() * 41
            at = hdr_off[last]
            idx = at[:, None] + T.arange(2, 6 + 125, device=dev, dtype=T.int64)[None, :]
            row = T.tensor(list(b"\0\0\0\0" + body), dtype=T.uint8, device=dev)
            wire[idx.reshape(-1)] = row.repeat(idx.shape[0])
        return wire, wire_len, hdr_off.contiguous()

    def timed(fns):
        """Alternating: one call of each per round; -> a stats dict per function."""
        ev = [[] for _ in fns]
        for _ in range(calls):
            for k, fn in enumerate(fns):
                e0, e1 = T.cuda.Event(enable_timing=True), T.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                ev[k].append((e0, e1))
        T.cuda.synchronize()
        out = []
        for pairs in ev:
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
            out.append({"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4),
                        "max_ms": round(ms[-1], 4)})
        return out

    def measure(with_close):
        wire, wire_len, hdr_off = build(with_close)
        desc = T.empty((n, 2), dtype=T.int64, device=dev)
        flags = T.empty(n, dtype=T.int16, device=dev)
        err = T.empty(n, dtype=T.uint8, device=dev)
        first = T.arange(0, n + 1, per, dtype=T.int32, device=dev)
        out_p = T.empty(n, dtype=T.uint8, device=dev)
        out_u = T.empty(n, dtype=T.uint8, device=dev)
        co = T.empty((ns, 8), dtype=T.uint8, device=dev)
        ws_h = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
        ws_p = kmws.Workspace(kmws.proto_workspace_size(n, ns))
        ws_u = kmws.Workspace(kmws.utf8_workspace_size(wire_len, n, ns))

        def unpack():
            kmws.unpack_headers(wire, hdr_off, kmws.SERVER, desc, flags, err, ws_h, wire_len=wire_len)

        def proto():
            kmws.proto_check(wire, desc, flags, out_p, ws_p, err=err, span=wire_len, masked=True, stream_first=first,
                             carry_out=co)

        def utf8():
            kmws.utf8_validate(wire, desc, flags, out_u, ws_u, span=wire_len, masked=True, stream_first=first)

        fns = (proto, utf8, unpack)
        for _ in range(a.warmup):
            for fn in fns:
                fn()
        r = timed(fns)
        assert ws_h.status() == 0 and ws_p.status() == 0 and ws_u.status() == 0
        assert not bool(err.any()), "the wire does not parse"
        assert bool((out_p == kmws.PROTO_OK).all()), "wrong verdicts at the benchmark size"
        assert bool((out_u == kmws.UTF8_NOT_TEXT).all())
        want_state = 2 if with_close else 0
        assert bool((co[:, 0] == want_state).all()) and not bool(co[:, 1:].any())
        return dict(zip(("proto_check", "utf8_validate_binary", "unpack_headers"), r)), wire_len

    res = {"tool": "bench_proto", "device": T.cuda.get_device_name(0), "frames": n, "streams": ns,
           "payload_bytes": "1-300", "calls": calls, "warmup": a.warmup, "order": "alternating"}
    main_r, wire_len = measure(False)
    res["wire_bytes"] = wire_len
    res.update(main_r)
    p, u = res["proto_check"]["median_ms"], res["utf8_validate_binary"]["median_ms"]
    res["proto_check"]["ns_per_frame"] = round(p * 1e6 / n, 4)
    res["proto_over_utf8_binary"] = round(p / u, 4)
    res["proto_within_utf8_binary"] = p <= u
    close_r, _ = measure(True)
    res["with_close_every_128th"] = close_r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["proto_within_utf8_binary"] else 1


if __name__ == "__main__":
    sys.exit(main())
