// The message rule of one stream's frames, stated once for the device scan
// (kmws_msg.hip: kmws_msg_index).  Plain __host__ __device__ functions:
// tests/cpp/msg_rule_check.cpp runs the very functions the kernels call.
//
// It is kmws_utf8_validate's message rule.  Per stream, in frame order, with b0
// = header byte 0 (fin << 7 | rsv << 4 | opcode):
//   opcode >= 8 (control): not a member, the state is unchanged;
//   opcode 1-7 (a head): starts a message -- an unfinished one keeps its record
//     without END -- and is its first member; with FIN the state goes to none,
//     else to open with b0 & 0x7F kept;
//   opcode 0 while a message is open: a member; FIN closes the message.  If it is
//     the message's first member in this batch (the message is open through the
//     carry) the record starts here;
//   opcode 0 while none is open (an orphan): not a member, the state is unchanged.
//
// Scan A, the state before each frame.  The state is one byte (0: none, else
// 0x80 | b0 of the open message's head) and one bit, `seen`: a frame with an
// opcode below 8 came before in this stream and batch.  While a message is open
// every such frame is a member, so an open state with `seen` clear is a message
// open through the carry that has no member in this batch yet: a CONTINUE there
// starts its record.  What a frame does to (state, seen) is two last-writer
// words side by side: it sets the state byte or keeps it, and it sets, clears or
// keeps `seen`.  They compose associatively, and a stream's first frame is
// composed behind the constant of its carry, which absorbs everything in front
// of it.  An orphan CONTINUE with FIN "sets" the state to none, which it already is.
//
// Scan B, everything else.  From the state before it a frame's class follows
// (member, starts a record, FIN); a record's totals are a segmented sum that is
// reset where a record starts and at a stream's first frame.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "kmws_gpu.h"
#include "kmws_utf8_rule.hpp"

namespace kmws {

// kScanBlockFrames (kmws_stream_scan.hpp; kmws_msg.hip ties them), exported for the tests, which read this line.
constexpr uint32_t kMsgBlockFrames = 1024;

// ---- scan A ----
constexpr uint32_t kMsgOpen = 0x80u;       // the state byte of an open message: kMsgOpen | b0 & 0x7F
constexpr uint32_t kMsgStateBits = 0xFFu;
constexpr uint32_t kMsgSet = 0x100u;       // the function sets the state byte (bits 0-7)
constexpr uint32_t kMsgSeenSet = 0x200u;   // it sets `seen` ...
constexpr uint32_t kMsgSeenClear = 0x400u; // ... or clears it (neither: keeps it)
constexpr uint32_t kMsgFnBits = 0x7FFu;

KMWS_HD uint32_t msg_identity() { return 0u; }
// a, then b
KMWS_HD uint32_t msg_compose(uint32_t a, uint32_t b)
{
    const uint32_t st = kMsgSet | kMsgStateBits, seen = kMsgSeenSet | kMsgSeenClear;
    return (((b & kMsgSet) ? b : a) & st) | (((b & seen) ? b : a) & seen);
}
// A stream's carried state: nothing before it matters.
KMWS_HD uint32_t msg_const(uint32_t state) { return kMsgSet | kMsgSeenClear | (state & kMsgStateBits); }
KMWS_HD uint32_t msg_frame_fn(uint32_t b0)
{
    const uint32_t op = b0 & 15u;
    if (op >= 8u) return msg_identity();
    if (op != 0u) return kMsgSet | kMsgSeenSet | ((b0 & 0x80u) ? 0u : kMsgOpen | (b0 & 0x7Fu));
    return kMsgSeenSet | ((b0 & 0x80u) ? kMsgSet : 0u);
}
// (state, seen) behind a function that is a constant (everything from a stream's first frame on is).
KMWS_HD uint32_t msg_state_of(uint32_t f) { return f & kMsgStateBits; }
KMWS_HD bool msg_seen_of(uint32_t f) { return (f & kMsgSeenSet) != 0u; }
// The general case, for the host check.
KMWS_HD uint32_t msg_apply_state(uint32_t f, uint32_t state) { return (f & kMsgSet) ? f & kMsgStateBits : state; }
KMWS_HD bool msg_apply_seen(uint32_t f, bool seen) { return (f & kMsgSeenSet) ? true : ((f & kMsgSeenClear) ? false : seen); }

// The carry: all zero = none; b[0] = 0x80 | b0, b[1..7] = 0, b[8..15] = the message's bytes so far.
KMWS_HD bool msg_carry_ok(const kmws_msg_carry& c)
{
    uint32_t rest = 0;
    for (int k = 1; k < 8; ++k) rest |= c.b[k];
    return rest == 0u && (c.b[0] == 0u || (c.b[0] & kMsgOpen));
}
KMWS_HD uint32_t msg_carry_state(const kmws_msg_carry& c) { return (c.b[0] & kMsgOpen) ? c.b[0] : 0u; }
KMWS_HD uint64_t msg_carry_prior(const kmws_msg_carry& c)
{
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v |= (uint64_t)c.b[8 + k] << (8 * k);
    return v;
}
KMWS_HD kmws_msg_carry msg_carry_make(uint32_t state, uint64_t bytes)
{
    kmws_msg_carry c;
    for (int k = 0; k < 16; ++k) c.b[k] = (uint8_t)0;
    if (state & kMsgOpen) {
        c.b[0] = (uint8_t)state;
        for (int k = 0; k < 8; ++k) c.b[8 + k] = (uint8_t)(bytes >> (8 * k));
    }
    return c;
}

// ---- a frame's class, the state before it known ----
constexpr uint32_t kMsgMember = 1u, kMsgStart = 2u, kMsgFin = 4u;  // FIN of a member
KMWS_HD uint32_t msg_class(uint32_t state, bool seen, uint32_t b0)
{
    const uint32_t op = b0 & 15u, fin = (b0 & 0x80u) ? kMsgFin : 0u;
    if (op >= 8u) return 0u;
    if (op != 0u) return kMsgMember | kMsgStart | fin;
    if (!(state & kMsgOpen)) return 0u;
    return kMsgMember | (seen ? 0u : kMsgStart) | fin;
}

// ---- scan B ----
// The records started so far and the running record's totals.  Canonical form:
// first == 0 unless the value holds a start, last == 0 unless it holds a member.
constexpr uint32_t kMsgSumReset = 0x80000000u;  // in `starts`: the value holds a reset point
constexpr uint32_t kMsgSumFin = 0x80000000u;    // in `frames`: one of the members has FIN
constexpr uint32_t kMsgSumCount = 0x7FFFFFFFu;  // the counts: a batch has fewer than 2^31 frames
struct MsgSum {
    uint32_t starts;  // records started | kMsgSumReset
    uint32_t first;   // the running record's first member
    uint32_t last;    // its last member so far
    uint32_t frames;  // its members so far | kMsgSumFin
    uint64_t bytes;   // their payload bytes
};
KMWS_HD MsgSum msg_sum_identity() { return MsgSum{0u, 0u, 0u, 0u, 0ull}; }
// a, then b
KMWS_HD MsgSum msg_sum_compose(const MsgSum& a, const MsgSum& b)
{
    // Every field chosen as a value, never as one of two references: the
    // compiler then keeps the sums in registers.
    const bool reset = (b.starts & kMsgSumReset) != 0u, b_has = (b.frames & kMsgSumCount) != 0u;
    const uint32_t first_a = a.first, first_b = b.first, last_a = a.last, last_b = b.last;
    const uint32_t frames_a = a.frames, frames_b = b.frames;
    const uint64_t bytes_a = a.bytes, bytes_b = b.bytes;
    MsgSum r;
    r.starts = (((a.starts & kMsgSumCount) + (b.starts & kMsgSumCount)) & kMsgSumCount) |
               ((a.starts | b.starts) & kMsgSumReset);
    r.first = reset ? first_b : first_a;
    r.last = (reset || b_has) ? last_b : last_a;
    r.frames = reset ? frames_b
                     : ((((frames_a & kMsgSumCount) + (frames_b & kMsgSumCount)) & kMsgSumCount) |
                        ((frames_a | frames_b) & kMsgSumFin));
    r.bytes = reset ? bytes_b : bytes_a + bytes_b;
    return r;
}
// Frame i of class `cls` with len payload bytes; stream_first: it is its stream's first frame.
KMWS_HD MsgSum msg_sum_of(uint32_t cls, bool stream_first, uint32_t i, uint32_t len)
{
    MsgSum e = msg_sum_identity();
    if (cls & kMsgMember) e.last = i, e.frames = 1u | ((cls & kMsgFin) ? kMsgSumFin : 0u), e.bytes = len;
    if (cls & kMsgStart) e.starts = 1u | kMsgSumReset, e.first = i;
    else if (stream_first) e.starts = kMsgSumReset;
    return e;
}
KMWS_HD uint32_t msg_sum_starts(const MsgSum& v) { return v.starts & kMsgSumCount; }
KMWS_HD uint32_t msg_sum_frames(const MsgSum& v) { return v.frames & kMsgSumCount; }

// The record of the running message of `v` (msg_sum_frames(v) != 0), everything
// but the fields read through `last`.  b0_first: header byte 0 of frame v.first;
// carry: its stream's carried state (read only when that frame is a CONTINUE).
KMWS_HD kmws_msg msg_record(const MsgSum& v, uint32_t stream, uint32_t b0_first, const kmws_msg_carry& carry)
{
    const bool begin = (b0_first & 15u) != 0u;
    kmws_msg m;
    m.off = 0, m.bytes = v.bytes, m.prior = begin ? 0ull : msg_carry_prior(carry);
    m.stream = stream, m.first = v.first, m.last = v.last, m.frames = msg_sum_frames(v);
    m.b0 = (uint8_t)((begin ? b0_first : msg_carry_state(carry)) & 0x7Fu);
    m.bits = (uint8_t)((begin ? KMWS_MSG_BEGIN : 0u) | ((v.frames & kMsgSumFin) ? KMWS_MSG_END : 0u));
    m.utf8 = m.proto = (uint8_t)0, m.reserved = 0u;
    return m;
}
// The stream's state after its last frame: v = the inclusive value there, rec =
// msg_record(v, ..) when the stream has a member in this batch.
KMWS_HD kmws_msg_carry msg_carry_after(const MsgSum& v, const kmws_msg& rec, const kmws_msg_carry& carry_in)
{
    if (msg_sum_frames(v) == 0u) return carry_in;
    if (rec.bits & KMWS_MSG_END) return msg_carry_make(0u, 0ull);
    return msg_carry_make(kMsgOpen | rec.b0, rec.prior + rec.bytes);
}

}  // namespace kmws
