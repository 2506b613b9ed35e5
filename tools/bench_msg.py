#!/usr/bin/env python3
"""Times kmws_msg_index on one MI355X and prints one JSON line.

The batch is tools/bench_proto.py's: 8,388,608 chat-sized frames (1-300 B
payloads, masked) of 65,536 streams, 128 frames each, laid out as a server-mode
wire on the device: seven of eight messages are one FIN BINARY frame, the
eighth is a BINARY head and a CONTINUE.  kmws_unpack_headers parses it once;
its out_desc / out_flags are what the timed calls get.  The index also gets a
pos array (the dense positions a gather's dst_off would hold), both verdict
arrays, msg_of, stream_msg_first and carry_out: every input and output it has.

Timed, whole calls, alternating in one process, device events, medians of
--calls (>= 20) each:
  kmws_msg_index      (five launches, 2 B of elements per frame);
  kmws_proto_check    (three launches) -- recorded, no bar;
  kmws_utf8_validate  on the same batch -- every message is binary, so this is
                      the cost of the project's other per-frame segmented scan.
The bar: the index takes no longer than that validate call
("msg_within_utf8_binary"; the exit status is 1 otherwise).

Then the same frames as 16-fragment messages (a BINARY head, 14 CONTINUEs, a
FIN CONTINUE; eight messages a stream): recorded, no bar.

    python tools/bench_msg.py [--frames 8388608] [--streams 65536] [--calls 20] [--out FILE]
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
    import numpy as np
    import torch as T
    from kuma_amd import kmws
    if kmws.device_count() < 1:
        print("bench_msg: no gfx950 device (nothing is measured without one)", file=sys.stderr)
        return 2
    calls = max(a.calls, 20)
    n, ns = a.frames, a.streams
    per = n // ns
    assert per * ns == n and per % 16 == 0, "whole streams of whole 16-frame groups"
    dev = "cuda"

    def build(fragments):
        """-> (wire, wire_len, hdr_off, lens, messages): the wire on the device."""
        g = T.Generator(device=dev)
        g.manual_seed(6455)
        lens = T.randint(1, 301, (n,), device=dev, generator=g, dtype=T.int64)
        pos = T.arange(n, device=dev, dtype=T.int64) % per
        if fragments == 16:
            b0 = T.full((n,), 0x00, dtype=T.int64, device=dev)
            b0[pos % 16 == 0] = 0x02
            b0[pos % 16 == 15] = 0x80
            messages = n // 16
        else:
            b0 = T.full((n,), 0x82, dtype=T.int64, device=dev)
            b0[pos % 8 == 0] = 0x02  # a BINARY head ...
            b0[pos % 8 == 1] = 0x80  # ... and its CONTINUE
            messages = n // 8 * 7
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
        # the mask keys: whatever the fill left (0x61616161) -- no payload is looked at
        return wire, wire_len, hdr_off.contiguous(), lens, messages

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

    def measure(fragments):
        wire, wire_len, hdr_off, lens, messages = build(fragments)
        desc = T.empty((n, 2), dtype=T.int64, device=dev)
        flags = T.empty(n, dtype=T.int16, device=dev)
        err = T.empty(n, dtype=T.uint8, device=dev)
        first = T.arange(0, n + 1, per, dtype=T.int32, device=dev)
        out_p = T.empty(n, dtype=T.uint8, device=dev)
        out_u = T.empty(n, dtype=T.uint8, device=dev)
        co_p = T.empty((ns, 8), dtype=T.uint8, device=dev)
        dense = (T.cumsum(lens, 0) - lens).contiguous()
        msgs = T.empty(messages * 48, dtype=T.uint8, device=dev)
        count = T.zeros(1, dtype=T.int32, device=dev)
        msg_of = T.empty(n, dtype=T.int32, device=dev)
        smf = T.empty(ns + 1, dtype=T.int32, device=dev)
        co_m = T.empty((ns, 16), dtype=T.uint8, device=dev)
        ws_h = kmws.Workspace(kmws.lib().kmws_unpack_workspace_size())
        ws_p = kmws.Workspace(kmws.proto_workspace_size(n, ns))
        ws_u = kmws.Workspace(kmws.utf8_workspace_size(wire_len, n, ns))
        ws_m = kmws.Workspace(kmws.msg_workspace_size(n, ns))
        kmws.unpack_headers(wire, hdr_off, kmws.SERVER, desc, flags, err, ws_h, wire_len=wire_len)
        assert ws_h.status() == 0 and not bool(err.any()), "the wire does not parse"

        def index():
            kmws.msg_index(desc, flags, msgs, count, ws_m, pos=dense, utf8=out_u, proto=out_p, stream_first=first,
                           carry_out=co_m, msg_of=msg_of, stream_msg_first=smf)

        def proto():
            kmws.proto_check(wire, desc, flags, out_p, ws_p, err=err, span=wire_len, masked=True, stream_first=first,
                             carry_out=co_p)

        def utf8():
            kmws.utf8_validate(wire, desc, flags, out_u, ws_u, span=wire_len, masked=True, stream_first=first)

        fns = (index, proto, utf8)
        for _ in range(a.warmup):
            for fn in fns[::-1]:  # the verdict arrays hold verdicts before the first index call
                fn()
        r = timed(fns)
        assert ws_p.status() == 0 and ws_u.status() == 0 and ws_m.status() == 0
        assert bool((out_p == kmws.PROTO_OK).all()) and bool((out_u == kmws.UTF8_NOT_TEXT).all())
        # the table at the benchmark size: every message whole, contiguous, in order
        m = msgs.cpu().numpy().view(kmws.msg_dtype())
        assert int(count.item()) == messages == m.shape[0], "wrong record count at the benchmark size"
        whole = kmws.MSG_BEGIN | kmws.MSG_END | kmws.MSG_CONTIG
        assert bool((m["bits"] == whole).all()) and bool((m["b0"] == 2).all()) and not m["prior"].any()
        assert int(m["frames"].sum()) == n and int(m["bytes"].sum()) == int(lens.sum().item())
        assert bool((m["first"][1:] == m["last"][:-1] + 1).all()) and m["first"][0] == 0
        assert bool((m["off"] == dense.cpu().numpy().view("u8")[m["first"]]).all())
        assert bool((m["stream"] == m["first"] // per).all())
        assert bool((msg_of.cpu().numpy()[m["last"]] == np.arange(messages)).all())
        assert bool((smf.cpu().numpy() == np.arange(ns + 1) * (messages // ns)).all())
        assert not bool(co_m.any())
        return dict(zip(("msg_index", "proto_check", "utf8_validate_binary"), r)), wire_len, messages

    res = {"tool": "bench_msg", "device": T.cuda.get_device_name(0), "frames": n, "streams": ns,
           "payload_bytes": "1-300", "calls": calls, "warmup": a.warmup, "order": "alternating"}
    main_r, wire_len, messages = measure(2)
    res["wire_bytes"], res["messages"] = wire_len, messages
    res.update(main_r)
    m, p, u = (res[k]["median_ms"] for k in ("msg_index", "proto_check", "utf8_validate_binary"))
    res["msg_index"]["ns_per_frame"] = round(m * 1e6 / n, 4)
    res["msg_over_utf8_binary"] = round(m / u, 4)
    res["msg_over_proto"] = round(m / p, 4)
    res["msg_within_utf8_binary"] = m <= u
    frag_r, _, frag_messages = measure(16)
    frag_r["messages"] = frag_messages
    res["fragments_16"] = frag_r
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["msg_within_utf8_binary"] else 1


if __name__ == "__main__":
    sys.exit(main())
