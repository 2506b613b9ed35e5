"""What the protocol-check tests share beside the model (proto_ref.py): the
frames-per-block constant read from the header that exports it, and the upload
of a proto_ref.device_batch to the device with one kmws_proto_check call."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_frames() -> int:
    """kProtoBlockFrames (kuma_amd/csrc/kmws_proto_rule.hpp): the frames one
    block of the device scan covers, and the aggregates one round of the
    aggregate scan covers."""
    txt = open(os.path.join(ROOT, "kuma_amd", "csrc", "kmws_proto_rule.hpp")).read()
    return int(re.search(r"constexpr uint32_t kProtoBlockFrames = (\d+);", txt).group(1))


GUARD = 4096


def run_gpu(batch, masked=False, rsv_allowed=0, use_err=True, carry_in=None, lo=0, hi=None, one_stream=False,
            span=None, keep=None):
    """kmws_proto_check on frames [lo, hi) of a proto_ref.device_batch (as one
    stream when one_stream, else with its stream_first).  The workspace lies
    between two guard regions and out is longer than n: both are checked, and
    that base is unchanged.  Returns (out, carry_out (ns,) states, status)."""
    import torch as T
    from kuma_amd import kmws
    hi = len(batch["off"]) if hi is None else hi
    n = hi - lo
    buf = np.frombuffer(batch["base"] + b"\0" * (-len(batch["base"]) % 16 or 16), dtype=np.uint8)
    span = len(batch["base"]) if span is None else span
    base = T.from_numpy(buf.copy()).cuda()
    descs = kmws.make_descs(np.array(batch["off"][lo:hi], dtype=np.int64), np.array(batch["len"][lo:hi], dtype=np.int64),
                            np.array(batch["key"][lo:hi], dtype=np.int64))
    fl = T.from_numpy(np.array(batch["flags"][lo:hi], dtype=np.int64).astype(np.int16)).cuda()
    err = T.from_numpy(np.array(batch["err"][lo:hi], dtype=np.uint8)).cuda() if use_err else None
    if n == 0:
        descs = T.zeros((0, 2), dtype=T.int64, device="cuda")
    out = T.full((n + 64,), 0xEE, dtype=T.uint8, device="cuda")
    if one_stream:
        sf, ns = None, 1
    else:
        assert lo == 0 and hi == len(batch["off"])
        first = batch["stream_first"]
        sf, ns = T.tensor(first, dtype=T.int32, device="cuda"), len(first) - 1
    ci = None
    if carry_in is not None:
        c = np.zeros((ns, 8), dtype=np.uint8)
        c[:, 0] = carry_in
        ci = T.from_numpy(c).cuda()
    co = T.full((ns, 8), 0xEE, dtype=T.uint8, device="cuda")
    need = kmws.proto_workspace_size(n, ns)
    guarded = T.full((need + 2 * GUARD,), 0xA7, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(0)
    ws.tensor = guarded[GUARD:GUARD + max(need, 16)]
    kmws.proto_check(base, descs, fl, out, ws, err=err, span=span, masked=masked, rsv_allowed=rsv_allowed,
                     stream_first=sf, carry_in=ci, carry_out=co)
    status = ws.status() if n else 0
    g = guarded.cpu().numpy()
    assert (g[:GUARD] == 0xA7).all() and (g[GUARD + max(need, 16):] == 0xA7).all(), "a guard region was written"
    assert np.array_equal(base.cpu().numpy(), buf), "the payload was written"
    o = out.cpu().numpy()
    assert (o[n:] == 0xEE).all(), "out was written past n"
    c = co.cpu().numpy()
    if status == 0:
        assert (c[:, 1:] == 0).all()
    if keep is not None:
        keep.update(base=base, descs=descs, fl=fl, err=err, out=out, ws=ws, sf=sf, ci=ci, co=co, guarded=guarded)
    return o[:n], c[:, 0].copy(), status


def expect(streams, rsv_allowed=0, carry_in=None, use_err=True):
    """The model's verdicts over all streams, flat, and the state after each."""
    import proto_ref as pr
    out, states = [], []
    for k, s in enumerate(streams):
        if not use_err:
            s = [f._replace(err=0) for f in s]
        v, st = pr.judge(s, rsv_allowed, 0 if carry_in is None else int(carry_in[k]))
        out += v
        states.append(st)
    return np.array(out, dtype=np.uint8), np.array(states, dtype=np.uint8)
