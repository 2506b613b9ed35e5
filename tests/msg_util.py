"""What the message-index tests share beside the model (msg_ref.py): the
frames-per-block constant read from the header that exports it, one guarded
kmws_msg_index call on streams of proto_ref frames, and the comparison of all
its outputs with the model's."""
import os
import re

import numpy as np

import msg_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block_frames() -> int:
    """kMsgBlockFrames (kuma_amd/csrc/kmws_msg_rule.hpp): the frames one block of
    the device scans covers, and the aggregates one round of an aggregate scan
    covers."""
    txt = open(os.path.join(ROOT, "kuma_amd", "csrc", "kmws_msg_rule.hpp")).read()
    return int(re.search(r"constexpr uint32_t kMsgBlockFrames = (\d+);", txt).group(1))


GUARD = 4096
SPARE = 3  # records behind msg_cap that must stay untouched


def flat(streams, lens=None):
    """-> (b0 per frame, payload length per frame, stream_first)."""
    b0 = [f.b0 for s in streams for f in s]
    if lens is None:
        lens = [len(f.payload) for s in streams for f in s]
    first = np.cumsum([0] + [len(s) for s in streams])
    return b0, list(lens), [int(x) for x in first]


def run_gpu(streams, pos=None, lens=None, carries=None, utf8=None, proto=None, one_stream=False, msg_cap=None,
            stream_first=None, outputs=True, keep=None):
    """kmws_msg_index on the streams' frames.  pos: a flat list -- the descriptors'
    offsets then hold other values -- or None: the call gets pos == NULL and the
    descriptors carry dense positions.  carries: 16 bytes per stream or None.
    one_stream: the frames as one stream without stream_first.  outputs=False:
    msg_of, stream_msg_first and carry_out are NULL.  The workspace lies between
    two guard regions, msgs has SPARE records behind msg_cap and msg_of is longer
    than n: all are checked.  -> dict(recs, count, msg_of, first_of, carries, status)."""
    import torch as T
    from kuma_amd import kmws
    b0, ln, first = flat(streams, lens)
    n = len(b0)
    dense = mr.dense_pos(streams, ln)
    off = np.array(dense, dtype=np.uint64) if pos is None else np.arange(n, dtype=np.uint64) * 7 + 0xDEAD0000
    descs = T.zeros((n, 2), dtype=T.int64, device="cuda")
    if n:
        d = np.zeros((n, 2), dtype=np.uint64)
        d[:, 0] = off
        d[:, 1] = np.array(ln, dtype=np.uint64) | (np.uint64(0xA5A5A5A5) << np.uint64(32))
        descs = T.from_numpy(d.view(np.int64)).cuda()
    fl = T.from_numpy((np.array(b0, dtype=np.int64) | 0x100).astype(np.int16)).cuda()
    d_pos = None if pos is None else T.from_numpy(np.array(pos, dtype=np.uint64).view(np.int64)).cuda()
    d_utf8 = None if utf8 is None else T.from_numpy(np.array(utf8, dtype=np.uint8)).cuda()
    d_proto = None if proto is None else T.from_numpy(np.array(proto, dtype=np.uint8)).cuda()
    if one_stream:
        sf, ns = None, 1
    else:
        first = first if stream_first is None else stream_first
        sf, ns = T.tensor(first, dtype=T.int32, device="cuda"), len(first) - 1
    ci = None
    if carries is not None:
        ci = T.from_numpy(np.frombuffer(b"".join(carries), dtype=np.uint8).reshape(ns, 16).copy()).cuda()
    co = T.full((ns, 16), 0xEE, dtype=T.uint8, device="cuda") if outputs else None
    cap = n if msg_cap is None else msg_cap
    msgs = T.full(((cap + SPARE) * 48,), 0xEE, dtype=T.uint8, device="cuda")
    count = T.full((2,), -1, dtype=T.int32, device="cuda")
    msg_of = T.full((n + 16,), 0x5A5A5A5A, dtype=T.int32, device="cuda") if outputs else None
    smf = T.full((ns + 1 + 16,), 0x5A5A5A5A, dtype=T.int32, device="cuda") if outputs else None
    need = kmws.msg_workspace_size(n, ns)
    guarded = T.full((max(need, 16) + 2 * GUARD,), 0xA7, dtype=T.uint8, device="cuda")
    ws = kmws.Workspace(0)
    ws.tensor = guarded[GUARD:GUARD + max(need, 16)]
    args = dict(pos=d_pos, utf8=d_utf8, proto=d_proto, stream_first=sf, carry_in=ci, carry_out=co, msg_of=msg_of,
                stream_msg_first=smf, msg_cap=cap)
    kmws.msg_index(descs, fl, msgs, count, ws, **args)
    status = ws.status() if n else 0
    g = guarded.cpu().numpy()
    assert (g[:GUARD] == 0xA7).all() and (g[GUARD + max(need, 16):] == 0xA7).all(), "a guard region was written"
    cnt = count.cpu().numpy()
    assert cnt[1] == -1
    raw = msgs.cpu().numpy()
    assert (raw[cap * 48:] == 0xEE).all(), "msgs was written past msg_cap"
    out = dict(count=int(cnt[0]), status=status, recs=raw[:min(int(cnt[0]), cap) * 48].view(kmws.msg_dtype()))
    if outputs:
        mo, sm = msg_of.cpu().numpy().view(np.uint32), smf.cpu().numpy().view(np.uint32)
        assert (mo[n:] == 0x5A5A5A5A).all() and (sm[ns + 1:] == 0x5A5A5A5A).all(), "an output was written past its end"
        c = co.cpu().numpy()
        out.update(msg_of=mo[:n], first_of=sm[:ns + 1], carries=[bytes(c[s]) for s in range(ns)])
    if keep is not None:
        keep.update(descs=descs, fl=fl, msgs=msgs, count=count, ws=ws, args=args, guarded=guarded)
    return out


def records_array(recs):
    from kuma_amd import kmws
    a = np.zeros(len(recs), dtype=kmws.msg_dtype())
    for name in mr.FIELDS:
        a[name] = [r[name] for r in recs]
    return a


def compare(got, want):
    """got: run_gpu's dict; want: msg_ref.walk's tuple."""
    recs, msg_of, first_of, after = want
    assert got["status"] == 0
    assert got["count"] == len(recs)
    w = records_array(recs)
    for name in mr.FIELDS + ("reserved",):
        bad = np.nonzero(got["recs"][name] != w[name])[0]
        assert bad.size == 0, (name, bad[:5], got["recs"][bad[:5]], w[bad[:5]])
    if "msg_of" in got:
        assert np.array_equal(got["msg_of"], np.array(msg_of, dtype=np.uint32))
        assert np.array_equal(got["first_of"], np.array(first_of, dtype=np.uint32))
        assert got["carries"] == list(after)


def check(streams, pos="dense", lens=None, carries=None, utf8=None, proto=None, **kw):
    """One call against the model.  pos: "dense" (a pos array of dense positions),
    None (pos == NULL, the descriptors' offsets) or a flat list."""
    _, ln, _ = flat(streams, lens)
    dense = mr.dense_pos(streams, ln)
    p = dense if pos is None or pos == "dense" else pos
    one = kw.get("one_stream", False)
    model_streams = [[f for s in streams for f in s]] if one else streams
    want = mr.walk(model_streams, p, ln, carries, utf8, proto)
    got = run_gpu(streams, pos=None if pos is None else p, lens=lens, carries=carries, utf8=utf8, proto=proto, **kw)
    compare(got, want)
    return got, want
