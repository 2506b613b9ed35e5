"""Host model of the batches tests/test_gpu_far_offsets.py runs past 2^31 and
2^32 bytes.  Plain numpy and the oracle: no torch, no GPU.

A batch is one PERIOD of P frames repeated `reps` times.  The oracle computes
every image of the period once (the masked wire, the unmasked wire, the encode
output, the gathered plain bytes, the reframed wire, the per-frame header
records, the UTF-8 verdicts of tests/utf8_ref.py); the device batch is

    source:  front | period | period | ...      stride S_src = wire + GAP
    output:  front image | period image | ...   stride S_out of the entry

with descriptor arrays built in numpy int64, off[i] = front + (i // P) * S +
poff[i % P], expected output offsets a numpy cumsum, and the expected bytes the
period image broadcast over `reps` rows.  Every stride is odd, so period k
starts at every residue mod 16 and 2^31 / 2^32 fall at unrelated places.

The front decides what lands on the boundary X (2^31 or 2^32): for the in-place
and wire-based entries it is `lead` gap bytes (the offset of the first period),
for the copy entries -- whose output starts at 0 -- one binary filler frame
whose length is chosen so that X in the OUTPUT lands where the lead's name
says.  tests/test_far_offset_cases.py proves on the CPU that the tiling is
valid and that every lead puts on X what it names."""
import random

import numpy as np

import pack_edge_cases as pec
import utf8_ref as ref
from oracle import oracle as orc

X31, X32 = 1 << 31, 1 << 32
MIN_SPAN = X32 + (1 << 27)
GAP = 38            # bytes between two periods in the source: S_src != every output stride
GAP_FILL = 0xA5     # gap and lead bytes (>= 0x80: never valid UTF-8 if a kernel read them as text)
MASK = 0x100
FILLER_B0 = 0x82    # the copy entries' front frame: FIN | BINARY
FILLER_KEY, FILLER_OUT_KEY = 0x00C0FFEE, 0x1BADB002
EURO = "€".encode()  # E2 82 AC

PACKED_WIRE_LENS = [0, 1, 7, 125, 126, 1000, 4096, 65535, 65536, 65537, 70001]

LEADS = ["payload_first_byte", "payload_last_byte_before", "header_straddles", "key_phase_1", "key_phase_2",
         "key_phase_3", "utf8_char_straddles", "utf8_fragment_edge", "utf8_bad_before", "utf8_bad_at", "utf8_bad_after"]
BAD_SHIFT = {"utf8_bad_before": 1, "utf8_bad_at": 0, "utf8_bad_after": -1}
SPACES = ("src", "gather", "encode", "reframe_m", "reframe_u")


def header_len(lens, mask):
    return pec.header_len(lens, mask)


def _plan(extra):
    """(length, role) per frame.  T/B: head of a text / binary message, t/b: a
    CONTINUE frame of one; the last frame of a message has FIN.  The messages
    the leads aim at are pinned, the other lengths are grouped at random."""
    rng = random.Random(len(extra))
    rest = [L for L in PACKED_WIRE_LENS if L not in (1000, 4096, 65537, 70001, 7, 125)] + list(extra)
    rng.shuffle(rest)
    plan = [(65537, "T"), (7, "t"), (125, "t"),   # the message of the char-straddle and bad-byte leads
            (70001, "B"),                          # payload / header / key-phase leads
            (1000, "T"), (4096, "t")]              # two fragments that split one code point
    while rest:
        k = min(len(rest), rng.randint(1, 3))
        kind = rng.choice("TTB")
        for j in range(k):
            plan.append((rest.pop(), kind if j == 0 else kind.lower()))
    return plan


class Period:
    """One period: frames, keys, payloads, and every image the oracle makes of them."""

    J_TEXT, J_BIG, J_EDGE = 0, 3, 4  # frames of _plan the leads aim at

    def __init__(self, name, extra, bad_at=None):
        self.name, self._extra = name, list(extra)
        plan = _plan(extra)
        self.P = P = len(plan)
        self.lens = np.array([L for L, _ in plan], dtype=np.int64)
        rng = random.Random(f"period-{name}")
        nrng = np.random.default_rng(len(extra) + 5)
        # header byte 0 per frame
        b0 = []
        for i, (L, role) in enumerate(plan):
            fin = i + 1 == P or plan[i + 1][1] in "TB"
            b0.append({"T": 1, "B": 2, "t": 0, "b": 0}[role] | (0x80 if fin else 0))
        self.b0 = np.array(b0, dtype=np.uint32)
        assert self.b0[0] & 0x0F and self.b0[-1] & 0x80  # starts with a message head, ends with FIN
        # payloads: well-formed text per text message (cut anywhere), random bytes for binary ones
        pay = [None] * P
        i = 0
        while i < P:
            j = i + 1
            while j < P and plan[j][1] in "tb":
                j += 1
            total = int(self.lens[i:j].sum())
            if plan[i][1] == "B":
                body = bytes(nrng.integers(0, 256, size=total, dtype=np.uint8))
            elif i == self.J_EDGE:
                body = ref.text(rng, 999) + EURO + ref.text(rng, total - 1002)  # E2 | 82 AC over the fragment edge
            else:
                body = ref.text(rng, total)
            for f in range(i, j):
                pay[f], body = body[:int(self.lens[f])], body[int(self.lens[f]):]
            i = j
        # the positions inside frame J_TEXT the UTF-8 leads aim at
        t = pay[self.J_TEXT]
        self.c3 = next(k for k in range(64, len(t) - 3) if 0xE0 <= t[k] <= 0xEF)      # a 3-byte code point
        self.c1 = next(k for k in range(self.c3 + 8, len(t) - 8)
                       if t[k] < 0x80 and t[k - 1] < 0x80 and t[k + 1] < 0x80)       # an ASCII byte
        self.bad_at, self._bad = bad_at, None
        if bad_at is not None:
            pay[self.J_TEXT] = t[:bad_at] + b"\xff" + t[bad_at + 1:]
        self.payloads = pay
        keys = nrng.integers(0, 2**32, size=P, dtype=np.uint64).astype(np.uint32)
        keys[5] = 0
        keys[self.J_BIG] = 0x7100A5C3  # a zero byte inside a key
        self.keys = keys
        self.out_keys = nrng.integers(0, 2**32, size=P, dtype=np.uint64).astype(np.uint32)
        self.enc_mask = (np.arange(P) % 3 != 1).astype(np.uint32)  # encode: masked and unmasked frames mixed
        self.enc_mask[self.J_BIG] = 1
        self._images()

    def bad_variant(self):
        """The same period with the ASCII byte c1 of frame J_TEXT replaced by FF."""
        if self._bad is None:
            self._bad = Period(self.name, self._extra, bad_at=self.c1)
        return self._bad

    def _images(self):
        P, lens = self.P, self.lens
        self.dense = np.frombuffer(b"".join(self.payloads), dtype=np.uint8).copy()
        self.doff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        dense16 = np.concatenate([self.dense, np.zeros(16, np.uint8)])
        self.flags_in = (self.b0 | MASK).astype(np.uint32)  # SERVER mode: every incoming frame is masked
        wire, woff = orc.encode_batch(dense16, self.doff, lens, self.flags_in, self.keys)
        self.hl = header_len(lens, 1)
        self.hdr_off = woff.astype(np.int64)
        self.pay_off = self.hdr_off + self.hl
        self.S_wire = len(wire)
        self.S_src = self.S_wire + GAP
        gap = np.full(GAP, GAP_FILL, np.uint8)
        self.src_masked = np.concatenate([wire, gap])
        plain = self.src_masked.copy()
        d = np.zeros(P, dtype=orc.DESC_DTYPE)
        d["off"], d["len"], d["key"] = self.pay_off, lens, self.keys
        orc.unmask_batch(plain, d)
        self.src_plain = plain
        self.verdicts = np.array(ref.validate_stream(list(zip(self.b0.tolist(), self.payloads)))[0], dtype=np.uint8)
        # output images: (bytes, header length per frame, flags passed for the outgoing frames)
        plain16 = np.concatenate([plain, np.zeros(16, np.uint8)])
        enc_flags = (self.b0 | (self.enc_mask << 8)).astype(np.uint32)
        enc_keys = np.where(self.enc_mask, self.out_keys, 0).astype(np.uint32)
        enc, _ = orc.encode_batch(plain16, self.pay_off, lens, enc_flags, enc_keys)
        rm, _ = orc.encode_batch(dense16, self.doff, lens, self.flags_in, self.out_keys)
        ru, _ = orc.encode_batch(dense16, self.doff, lens, self.b0, np.zeros(P, np.uint32))
        self.out = {
            "gather": (self.dense, np.zeros(P, np.int64), None),
            "encode": (enc, header_len(lens, self.enc_mask), enc_flags),
            "reframe_m": (rm, header_len(lens, 1), self.flags_in),
            "reframe_u": (ru, header_len(lens, 0), self.b0.copy()),
        }

    # ---- geometry of one image ----
    def geom(self, space):
        """(stride, hdr start, payload start per frame) of the period in `space`."""
        if space == "src":
            return self.S_src, self.hdr_off, self.pay_off
        img, hl, _ = self.out[space]
        sizes = hl + self.lens
        h = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        assert len(img) == int(sizes.sum())
        return len(img), h, h + hl

    def sizes(self, space):
        S, h, p = self.geom(space)
        return (p - h) + self.lens

    def target(self, space, lead):
        """The period offset in `space` that the lead puts on X."""
        S, h, p = self.geom(space)
        jb, jt, je = self.J_BIG, self.J_TEXT, self.J_EDGE
        if lead == "payload_first_byte":
            return int(p[jb])
        if lead == "payload_last_byte_before":
            return int(p[jb] + self.lens[jb])
        if lead == "header_straddles":
            assert p[jb] - h[jb] >= 10
            return int(p[jb]) - 2  # masked: 2 key bytes on each side; unmasked: inside the 64-bit length
        if lead.startswith("key_phase_"):
            return int(p[jb]) + 20 + int(lead[-1])
        if lead == "utf8_char_straddles":
            return int(p[jt]) + self.c3 + 1
        if lead == "utf8_fragment_edge":
            return int(p[je] + self.lens[je])
        return int(p[jt]) + self.c1 + BAD_SHIFT[lead]


def make_period(name):
    """chunk: the packed_wire mix + every phase-batch length (mean region < 16 KiB);
    unit: the packed_wire mix + four of them (mean region >= 16 KiB)."""
    extra = list(pec.PHASE_LENS) if name == "chunk" else [4097, 1025, 33, 17]
    extra[-1] += (sum(PACKED_WIRE_LENS) + sum(extra) + 1) % 2  # an odd payload total: every stride is odd
    return Period(name, extra)


_periods = {}


def period(name):
    if name not in _periods:
        _periods[name] = make_period(name)
    return _periods[name]


class Layout:
    """The device batch of (period, output space, lead, X): the front, reps,
    and the absolute arrays.  space == "src": an in-place / wire-based entry,
    the lead is gap bytes and aims at the source.  Any other space: a copy
    entry, the front is one filler frame and the lead aims at that output
    (the gather has no headers: its header_straddles aims at the source)."""

    def __init__(self, p, space, lead, X=X32, reps=None, min_span=MIN_SPAN):
        self.p, self.space, self.lead, self.X = p, space, lead, X
        self.copy = space != "src"
        self.aim = "src" if (not self.copy or (space == "gather" and lead == "header_straddles")) else space
        S_aim = p.geom(self.aim)[0]
        t = p.target(self.aim, lead)
        if not self.copy:
            self.front_src = (X - t) % S_aim
            self.f = None
        else:
            fh_out = {"gather": 0, "encode": 14, "reframe_m": 14, "reframe_u": 10}[space]
            fh_aim = 14 if self.aim == "src" else fh_out
            self.f = (X - t - fh_aim) % S_aim + S_aim  # the filler's payload: >= one period, a 64-bit length
            self.front_src = 14 + self.f
            self.front_out = fh_out + self.f
        S_out = p.geom(space)[0]
        if reps is None:
            reps = max(-(-(min_span - self.front_src) // p.S_src),
                       -(-(min_span - self.front_out) // S_out) if self.copy else 0) + 1
        self.reps = reps
        P = p.P
        self.nf = 1 if self.copy else 0  # frames of the front
        self.n = self.nf + reps * P
        k = np.repeat(np.arange(reps, dtype=np.int64), P)
        tile = lambda a: np.tile(np.asarray(a, dtype=np.int64), reps)
        front = lambda v: np.array([v] * self.nf, dtype=np.int64)
        self.hdr_off = np.concatenate([front(0), self.front_src + k * p.S_src + tile(p.hdr_off)])
        self.pay_off = np.concatenate([front(14), self.front_src + k * p.S_src + tile(p.pay_off)])
        self.lens = np.concatenate([front(self.f), tile(p.lens)])
        self.keys = np.concatenate([front(FILLER_KEY), tile(p.keys)])
        self.out_keys = np.concatenate([front(FILLER_OUT_KEY), tile(p.out_keys)])
        self.b0 = np.concatenate([front(FILLER_B0), tile(p.b0)])
        self.src_bytes = self.front_src + reps * p.S_src
        # the period that holds the invalid byte of a utf8_bad_* lead
        self.bad_row = None
        if lead in BAD_SHIFT:
            front_aim = self.front_src if self.aim == "src" else self.front_out
            self.bad_row = (X - front_aim) // S_aim
            assert 0 <= self.bad_row < reps
        self.verdicts = np.concatenate([np.zeros(self.nf, np.uint8), np.tile(p.verdicts, reps)])
        if self.bad_row is not None:
            a = self.nf + self.bad_row * P
            self.verdicts[a:a + P] = p.bad_variant().verdicts
        if self.copy:
            self.out_sizes = np.concatenate([front(self.front_out), tile(p.sizes(space))])
            self.out_off = np.concatenate([[0], np.cumsum(self.out_sizes)]).astype(np.int64)
            self.out_bytes = int(self.out_off[-1])
            hl = p.out[space][1]
            self.out_hl = np.concatenate([front(self.front_out - self.f), tile(hl)])

    # ---- flags the entries take ----
    def flags_in(self):
        return (self.b0 | MASK).astype(np.uint32)

    def flags_out(self):
        """Outgoing flags of the copy entry (encode: mixed masks; reframe: all / none)."""
        p, m = self.p, {"encode": None, "reframe_m": 1, "reframe_u": 0}[self.space]
        per = p.enc_mask if m is None else np.full(p.P, m, np.uint32)
        fm = 1 if self.space != "reframe_u" else 0
        return (self.b0 | (np.concatenate([[fm] * self.nf, np.tile(per, self.reps)]).astype(np.uint32) << 8)).astype(
            np.uint32)

    # ---- the front's bytes ----
    def filler_payload(self):
        return np.random.default_rng(self.f).integers(0, 256, size=self.f, dtype=np.uint8)

    def front_images(self):
        """(masked source front, plain source front, output front) as uint8 arrays."""
        if not self.copy:
            g = np.full(self.front_src, GAP_FILL, np.uint8)
            return g, g, None
        pay = np.concatenate([self.filler_payload(), np.zeros(16, np.uint8)])
        one = lambda fl, key: orc.encode_batch(pay, np.zeros(1, np.uint64), np.array([self.f]),
                                               np.array([fl], np.uint32), np.array([key], np.uint32))[0]
        masked = one(FILLER_B0 | MASK, FILLER_KEY)
        plain = np.concatenate([masked[:14], pay[:self.f]])
        out = {"gather": lambda: pay[:self.f].copy(),
               "encode": lambda: one(FILLER_B0 | MASK, FILLER_OUT_KEY),
               "reframe_m": lambda: one(FILLER_B0 | MASK, FILLER_OUT_KEY),
               "reframe_u": lambda: one(FILLER_B0, 0)}[self.space]()
        assert len(masked) == self.front_src and len(out) == self.front_out
        return masked, plain, out

    def period_images(self, row_bad=False):
        """(masked source, plain source, output image) of a period (of the bad one)."""
        q = self.p.bad_variant() if row_bad else self.p
        return q.src_masked, q.src_plain, (q.out[self.space][0] if self.copy else None)

    # ---- what lies on an absolute byte (the CPU proofs) ----
    def payload_byte(self, i, q):
        """Plain payload byte q of frame i."""
        if i < self.nf:
            return int(self.filler_payload()[q])
        row, j = divmod(i - self.nf, self.p.P)
        per = self.p.bad_variant() if row == self.bad_row else self.p
        return per.payloads[j][q]

    def aim_arrays(self):
        """(header start, payload start, length per frame) in the space the lead aims at."""
        if self.aim == "src":
            return self.hdr_off, self.pay_off, self.lens
        return self.out_off[:-1], self.out_off[:-1] + self.out_hl, self.lens
