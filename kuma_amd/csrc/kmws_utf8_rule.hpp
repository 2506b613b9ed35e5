// UTF-8 well-formedness as a byte rule with three bytes of look-back, and the
// per-frame message state the validator scans over a batch (kmws_utf8.hip).
// Plain __host__ __device__ functions: tests/cpp/utf8_rule_check.cpp runs the
// very functions the kernels call.
//
// RFC 3629 section 4 / Unicode table 3-7: no C0, C1, F5..FF; E0 is followed by
// A0..BF, ED by 80..9F, F0 by 90..BF, F4 by 80..8F; every other continuation
// is 80..BF.  While the bytes before a byte form a prefix of a well-formed
// string, what that byte may be depends on the last three of them only (the
// pending incomplete sequence is at most three bytes long), so "the first byte
// the rule rejects" is the first byte at which the message stops being such a
// prefix.  Look-back bytes that do not exist (message start) are 0: an ASCII
// byte leaves nothing pending.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#define KMWS_HD __host__ __device__ inline

namespace kmws {

// Look-back L: the last three message bytes, the most recent in bits 0-7.
KMWS_HD uint32_t utf8_append(uint32_t L, uint32_t b) { return ((L << 8) | (b & 0xFFu)) & 0xFFFFFFu; }

// What the next byte must be after look-back L: 0 = a code point starts (00..7F
// or a lead C2..F4), else lo | hi << 8 = a continuation in [lo, hi].
// Written without branches (range tests as one unsigned compare, & and | on 0 / 1
// values, selects): every lane of a wave runs the same instructions whatever its
// bytes are.  p1, p2, p3: the bytes one, two and three before.
KMWS_HD uint32_t utf8_need3(uint32_t p1, uint32_t p2, uint32_t p3)
{
    const uint32_t lead = (p1 - 0xC2u) <= 0x32u;     // C2..F4: its first continuation
    const uint32_t cont1 = (p1 & 0xC0u) == 0x80u;
    const uint32_t second = (p2 - 0xE0u) <= 0x14u;   // E0..F4 and one continuation: one of its 2 or 3
    const uint32_t third = (uint32_t)((p2 & 0xC0u) == 0x80u) & (uint32_t)((p3 - 0xF0u) <= 4u);  // F0..F4 and two
    const uint32_t need = lead | (cont1 & (second | third));
    // the narrowed ranges follow E0, ED, F0, F4 only: a continuation p1 leaves 80..BF
    const uint32_t lo = p1 == 0xE0u ? 0xA0u : (p1 == 0xF0u ? 0x90u : 0x80u);
    const uint32_t hi = p1 == 0xEDu ? 0x9Fu : (p1 == 0xF4u ? 0x8Fu : 0xBFu);
    return need ? (lo | (hi << 8)) : 0u;
}
KMWS_HD uint32_t utf8_need(uint32_t L) { return utf8_need3(L & 0xFFu, (L >> 8) & 0xFFu, (L >> 16) & 0xFFu); }

// Byte b after the bytes p1, p2, p3 (look-back L) breaks well-formedness.
KMWS_HD bool utf8_byte_bad3(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3)
{
    const uint32_t need = utf8_need3(p1, p2, p3);
    const uint32_t lo = need & 0xFFu, hi = need >> 8;
    const uint32_t bad_cont = (b - lo) > (hi - lo);
    const uint32_t bad_start = (uint32_t)(b >= 0x80u) & (uint32_t)((b - 0xC2u) > 0x32u);
    return (need ? bad_cont : bad_start) != 0u;
}
KMWS_HD bool utf8_byte_bad(uint32_t b, uint32_t L)
{
    return utf8_byte_bad3(b, L & 0xFFu, (L >> 8) & 0xFFu, (L >> 16) & 0xFFu);
}

// ---- the same rule on a 16-byte word, four bytes per operation ----
//
// Per dword, class masks with one bit per byte (its bit 7).  Every threshold is
// >= 80, so "byte >= K" is: bit 7 set, and the low seven bits >= K - 80 -- one
// subtraction on all four bytes ((x & 7F..) | 80.. minus a byte in 00..7F never
// borrows).  The mask of "the byte one / two / three before" is the mask shifted
// by bytes across the dword before.  A byte is in error when it is a
// continuation exactly where none is due (or the reverse), when it is C0, C1 or
// F5..FF, or when it breaks the narrowed range after E0 / ED / F0 / F4.  "Due"
// drops the rule's "and the bytes between are continuations": where that
// matters, the byte between is itself in error one or two bytes earlier, in
// this word or in the three bytes before it, which belong to the same frame --
// so a frame holds an error of this form iff it holds one of the byte rule
// (tests/cpp/utf8_rule_check.cpp checks exactly that on random windows).
struct Utf8Swar {
    uint32_t cont, lead234, lead34, lead4, e0, ed, f0, f4, bad, ge_a0, ge_90;
};
KMWS_HD Utf8Swar utf8_swar_classes(uint32_t x)
{
    const uint32_t hi = x & 0x80808080u, t = (x & 0x7F7F7F7Fu) | 0x80808080u;
#define KMWS_GE(K) (hi & (t - ((uint32_t)(K) - 0x80u) * 0x01010101u))
    const uint32_t c0 = KMWS_GE(0xC0), c2 = KMWS_GE(0xC2), e0 = KMWS_GE(0xE0), e1 = KMWS_GE(0xE1);
    const uint32_t ed = KMWS_GE(0xED), ee = KMWS_GE(0xEE), f0 = KMWS_GE(0xF0), f1 = KMWS_GE(0xF1);
    const uint32_t f4 = KMWS_GE(0xF4), f5 = KMWS_GE(0xF5);
    Utf8Swar c;
    c.ge_a0 = KMWS_GE(0xA0);
    c.ge_90 = KMWS_GE(0x90);
#undef KMWS_GE
    c.cont = hi & ~c0;
    c.lead234 = c2 & ~f5;
    c.lead34 = e0 & ~f5;
    c.lead4 = f0 & ~f5;
    c.e0 = e0 & ~e1;
    c.ed = ed & ~ee;
    c.f0 = f0 & ~f1;
    c.f4 = f4 & ~f5;
    c.bad = (c0 & ~c2) | f5;
    return c;
}
// The mask of the byte nb (1..3) bytes earlier, at each byte's own position.
KMWS_HD uint32_t utf8_swar_back(uint32_t cur, uint32_t before, uint32_t nb)
{
    return (cur << (8u * nb)) | (before >> (32u - 8u * nb));
}
KMWS_HD uint32_t utf8_swar_dword(const Utf8Swar& c, const Utf8Swar& p)
{
    const uint32_t due = utf8_swar_back(c.lead234, p.lead234, 1) | utf8_swar_back(c.lead34, p.lead34, 2) |
                         utf8_swar_back(c.lead4, p.lead4, 3);
    return (due ^ c.cont) | c.bad | (utf8_swar_back(c.e0, p.e0, 1) & ~c.ge_a0) |
           (utf8_swar_back(c.ed, p.ed, 1) & c.ge_a0) | (utf8_swar_back(c.f0, p.f0, 1) & ~c.ge_90) |
           (utf8_swar_back(c.f4, p.f4, 1) & c.ge_90);
}
// The word x0..x3 (memory order) after the dword `prev`, all inside one frame
// from three bytes before the word on: does it hold an error?
KMWS_HD bool utf8_word_bad_swar(uint32_t prev, uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3)
{
    const Utf8Swar cp = utf8_swar_classes(prev), c0 = utf8_swar_classes(x0), c1 = utf8_swar_classes(x1),
                   c2 = utf8_swar_classes(x2), c3 = utf8_swar_classes(x3);
    const uint32_t err = utf8_swar_dword(c0, cp) | utf8_swar_dword(c1, c0) | utf8_swar_dword(c2, c1) |
                         utf8_swar_dword(c3, c2);
    return (err & 0x80808080u) != 0u;
}

// A message whose last bytes are L ends inside a code point.
KMWS_HD bool utf8_pending(uint32_t L) { return utf8_need(L) != 0u; }

// ---- message state of one stream, and the scan over a batch's frames ----
//
// An element is what a run of consecutive frames does to the state of their
// stream: either it sets the state outright (`reset`: the run holds a message
// head, a closing FIN or a stream start with its carry) or it only appends
// payload bytes to the look-back of whatever message is open.  `slot` is the
// index in this batch of the frame the message's verdict word belongs to: its
// head, or the stream's first frame for a message carried in.
struct Utf8Elem {
    uint32_t slot;
    uint32_t w;  // look-back (bits 0-23) | bytes held, 0..3 (24-25) | open (26) | checked (27) | reset (28)
};
constexpr uint32_t kUtf8Open = 1u << 26, kUtf8Checked = 1u << 27, kUtf8Reset = 1u << 28;
KMWS_HD uint32_t utf8_elem_ctx(Utf8Elem e) { return e.w & 0xFFFFFFu; }
KMWS_HD uint32_t utf8_elem_nb(Utf8Elem e) { return (e.w >> 24) & 3u; }
KMWS_HD Utf8Elem utf8_identity() { return Utf8Elem{0u, 0u}; }

// a then b.  Associative: "concatenate and keep the last three, restart at a reset".
KMWS_HD Utf8Elem utf8_combine(Utf8Elem a, Utf8Elem b)
{
    if (b.w & kUtf8Reset) return b;
    const uint32_t nb = utf8_elem_nb(b), na = utf8_elem_nb(a);
    const uint32_t ctx = nb >= 3u ? utf8_elem_ctx(b) : (((utf8_elem_ctx(a) << (8u * nb)) | utf8_elem_ctx(b)) & 0xFFFFFFu);
    const uint32_t n = na + nb > 3u ? 3u : na + nb;
    return Utf8Elem{a.slot, ctx | (n << 24) | (a.w & (kUtf8Open | kUtf8Checked | kUtf8Reset))};
}

// Frame i with header byte 0 `op_byte` (fin << 7 | rsv1 << 6 | .. | opcode),
// whose last nb = min(len, 3) payload bytes are `tail` (the last in bits 0-7).
// A frame that closes its message keeps its own tail in the element: the
// state after it is "between messages", and the tail is what rule (b) needs.
KMWS_HD Utf8Elem utf8_frame_elem(uint32_t op_byte, uint32_t i, uint32_t tail, uint32_t nb)
{
    const uint32_t op = op_byte & 0x0Fu, fin = op_byte & 0x80u, rsv1 = op_byte & 0x40u;
    const uint32_t bytes = (tail & 0xFFFFFFu) | (nb << 24);
    if (op >= 8u) return utf8_identity();              // control: invisible
    if (fin) return Utf8Elem{i, bytes | kUtf8Reset};   // closes (a head that is its whole message too)
    if (op == 0u) return Utf8Elem{0u, bytes};          // CONTINUE: appends
    return Utf8Elem{i, bytes | kUtf8Reset | kUtf8Open | ((op == 1u && !rsv1) ? kUtf8Checked : 0u)};
}

// How frame i sees itself, given the state `before` it: checked or not, its
// message's slot, and the look-back at its first payload byte.
struct Utf8View {
    uint32_t slot;
    uint32_t w;  // look-back (bits 0-23) | checked (27)
};
KMWS_HD Utf8View utf8_frame_view(Utf8Elem before, uint32_t op_byte, uint32_t i)
{
    const uint32_t op = op_byte & 0x0Fu, rsv1 = op_byte & 0x40u;
    if (op >= 8u) return Utf8View{i, 0u};
    if (op != 0u) return Utf8View{i, (op == 1u && !rsv1) ? kUtf8Checked : 0u};
    if ((before.w & (kUtf8Open | kUtf8Checked)) != (kUtf8Open | kUtf8Checked)) return Utf8View{i, 0u};
    return Utf8View{before.slot, utf8_elem_ctx(before) | kUtf8Checked};
}

// ---- the 8-byte carry of a stream between two batches (kmws_utf8_carry) ----
// b[0]: bit 0 open, bit 1 checked, bit 2 already reported BAD; b[1..3]: the
// look-back, most recent byte first.  All zero: between messages.
constexpr uint32_t kUtf8CarryOpen = 1u, kUtf8CarryChecked = 2u, kUtf8CarryBad = 4u;
KMWS_HD uint64_t utf8_carry_pack(Utf8Elem after, bool bad)
{
    if (!(after.w & kUtf8Open)) return 0ull;
    if (!(after.w & kUtf8Checked)) return (uint64_t)kUtf8CarryOpen;
    return (uint64_t)(kUtf8CarryOpen | kUtf8CarryChecked | (bad ? kUtf8CarryBad : 0u)) |
           ((uint64_t)utf8_elem_ctx(after) << 8);
}
// The state a carry stands for, as the reset element in front of the stream's
// first frame `slot`; *bad: the message was already reported BAD.
KMWS_HD Utf8Elem utf8_carry_unpack(uint64_t c, uint32_t slot, bool* bad)
{
    const uint32_t f = (uint32_t)c & 0xFFu;
    *bad = (f & kUtf8CarryOpen) && (f & kUtf8CarryChecked) && (f & kUtf8CarryBad);
    if (!(f & kUtf8CarryOpen)) return Utf8Elem{slot, kUtf8Reset};
    if (!(f & kUtf8CarryChecked)) return Utf8Elem{slot, kUtf8Reset | kUtf8Open};
    return Utf8Elem{slot, ((uint32_t)(c >> 8) & 0xFFFFFFu) | (3u << 24) | kUtf8Reset | kUtf8Open | kUtf8Checked};
}

}  // namespace kmws
