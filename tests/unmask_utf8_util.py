"""Shared helpers of tests/test_gpu_unmask_utf8.py: batches in the style of
tests/test_gpu_utf8.py (its Batch: plain payloads placed in an arena whose gaps
hold bytes >= 0x80), the fused call, and the three things every case asserts --
the whole arena, the verdicts, the status."""
import random

import numpy as np

import test_gpu_utf8 as vt
import utf8_ref as ref

Batch, T_, C_, B_, FIN, RSV1, PING = vt.Batch, vt.T_, vt.C_, vt.B_, vt.FIN, vt.RSV1, vt.PING


def nonzero_keys(batch):
    """Every frame masked: Batch leaves each 17th key 0."""
    batch.keys[batch.keys == 0] = np.uint32(0x5A17C3E9)
    return batch


def expected_arena(batch, lo=0, hi=None):
    """The arena after a call on frames [lo, hi): those plain, every other byte
    as the masked arena holds it (gaps and the rounding tail included)."""
    hi = batch.n if hi is None else hi
    if lo == 0 and hi == batch.n:
        return batch.plain
    buf = batch.masked()
    for o, L in zip(batch.offs[lo:hi], batch.lens[lo:hi]):
        buf[o:o + L] = batch.plain[o:o + L]
    return buf


def device_inputs(batch, lo=0, hi=None, stream_first=None, carry_in=None):
    import torch as T
    from kuma_amd import kmws
    hi = batch.n if hi is None else hi
    n = hi - lo
    ns = 1 if stream_first is None else len(stream_first) - 1
    return dict(
        n=n, ns=ns, masked=T.from_numpy(batch.masked()).cuda(),
        descs=kmws.make_descs(batch.offs[lo:hi], batch.lens[lo:hi], batch.keys[lo:hi].astype(np.int64)),
        fl=T.from_numpy(batch.flags[lo:hi].astype(np.int16)).cuda(),
        sf=None if stream_first is None else T.tensor(list(stream_first), dtype=T.int32, device="cuda"),
        ci=None if carry_in is None else T.from_numpy(np.ascontiguousarray(carry_in, dtype=np.uint8)).cuda(),
        ws=kmws.Workspace(kmws.unmask_utf8_workspace_size(batch.total, n, ns)))


def run_fused(batch, stream_first=None, carry_in=None, lo=0, hi=None, schedule=None, dev=None):
    """kmws_unmask_utf8_batch on frames [lo, hi) of the masked batch; returns
    (arena afterwards, out, carry_out, status)."""
    import torch as T
    from kuma_amd import kmws
    dev = dev or device_inputs(batch, lo, hi, stream_first, carry_in)
    n, ns = dev["n"], dev["ns"]
    base = dev["masked"].clone()
    out = T.full((max(n, 1),), 0xEE, dtype=T.uint8, device="cuda")
    co = T.full((max(ns, 1), 8), 0xEE, dtype=T.uint8, device="cuda")
    kmws.unmask_utf8(base, dev["descs"], dev["fl"], out, dev["ws"], span=batch.total, stream_first=dev["sf"],
                     carry_in=dev["ci"], carry_out=co, schedule=schedule)
    status = dev["ws"].status() if n else 0
    return base.cpu().numpy(), out.cpu().numpy()[:n], co.cpu().numpy()[:ns], status


def check_fused(batch, expect=None, **kw):
    """(i) the whole arena, (ii) the verdicts against the reference, (iii) status 0."""
    expect = vt.want(batch.frames) if expect is None else np.asarray(expect, dtype=np.uint8)
    arena, out, carry, st = run_fused(batch, **kw)
    assert st == 0
    want = expected_arena(batch)
    diff = np.nonzero(arena != want)[0]
    assert diff.size == 0, ("arena", diff[:10], arena[diff[:10]], want[diff[:10]])
    bad = np.nonzero(out != expect)[0]
    assert bad.size == 0, ("verdicts", bad[:10], out[bad[:10]], expect[bad[:10]])
    return expect, carry


def sweep_batch(o, aligned):
    """The boundary sweep of tests/test_gpu_utf8.py::test_boundary_sweep: the
    40 KiB text at arena offsets o (+ 64 KiB multiples, or packed), each copy
    but the first with one corruption within +-4 bytes of a 16 B / 1 KiB /
    4 KiB / 16 KiB boundary.  Returns (batch, expected verdicts, cases per class)."""
    data, arr = vt.sweep_text()
    rng = random.Random(100 + o)
    if aligned:
        plan = [None] + vt.sweep_copies(o)
        copies = [(j * 65536 + o, c) for j, c in enumerate(plan)]
    else:
        copies, pos = [(o, None)], o + vt.SWEEP_LEN
        for j in range(len(vt.sweep_copies(o))):
            off = pos + rng.randint(2, 14)
            cands = vt.sweep_copies(off)
            copies.append((off, cands[j % len(cands)]))
            pos = off + vt.SWEEP_LEN
    total = copies[-1][0] + vt.SWEEP_LEN + 7
    b = Batch([(T_ | FIN, data)] * len(copies), [c[0] for c in copies], total)
    expect, classes = [], {}
    for off, c in copies:
        if c is None:
            expect.append(ref.OK)
            continue
        unit, p, newb = c
        b.plain[off + p] = newb
        expect.append(vt.sweep_verdict(b.plain[off:off + vt.SWEEP_LEN], p))
        classes[unit] = classes.get(unit, 0) + 1
    return b, expect, classes


def wide_text(width, nbytes, seed):
    """nbytes (a multiple of width) of well-formed UTF-8 made only of code
    points `width` (3 or 4) bytes wide, as a uint8 array."""
    rng = np.random.default_rng(seed)
    k = nbytes // width
    assert k * width == nbytes
    if width == 3:
        cp = rng.integers(0x800, 0xD800, size=k, dtype=np.uint32)
        cols = [0xE0 | (cp >> 12), 0x80 | ((cp >> 6) & 0x3F), 0x80 | (cp & 0x3F)]
    else:
        cp = rng.integers(0x10000, 0x110000, size=k, dtype=np.uint32)
        cols = [0xF0 | (cp >> 18), 0x80 | ((cp >> 12) & 0x3F), 0x80 | ((cp >> 6) & 0x3F), 0x80 | (cp & 0x3F)]
    data = np.stack(cols, axis=1).astype(np.uint8).reshape(-1)
    bytes(data).decode("utf-8")  # valid by construction; confirmed
    return data


def mix_counts(streams, per_stream):
    """(OK messages, BAD messages, NOT_TEXT frames, frames) on the reference's verdicts."""
    ok, bad, _ = vt.fuzz_mix(streams, per_stream)
    verdicts = [v for r in per_stream for v in r]
    return ok, bad, sum(v == ref.NOT_TEXT for v in verdicts), len(verdicts)
