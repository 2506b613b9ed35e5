// The UTF-8 message state of ONE connection on the host path (kmws_decoder_feed,
// kmws_decoder_feed_deferred / kmws_rx_batch_*): what kmws_utf8_validate gets
// from its five-kernel scan over a batch, the host decoder gets from a few
// instructions per frame, because it walks each connection's frames in order
// anyway and sees every payload when it queues it.  Host-only, plain inline
// functions over kmws_utf8_rule.hpp (the rule is stated there, once);
// tests/cpp/utf8_stream_check.cpp drives exactly these.
//
// Two halves:
//  - at PARSE time (a frame is complete, its payload contiguous in host memory):
//    utf8_stream_frame turns header byte 0 and the frame's last min(len, 3)
//    plain payload bytes into the frame's view -- checked?, message head?, the
//    24-bit look-back at its first payload byte, "this FIN leaves a code point
//    pending" (rule (b), which an empty frame can trigger) -- and advances the
//    stream's state.  The payload pass on the device needs the look-back and the
//    checked bit only, and answers with one bad bit per frame;
//  - at DELIVERY time, in frame order: utf8_stream_verdict turns the view and
//    the device's bad bit into KMWS_UTF8_* and remembers which message was
//    already reported BAD.
// A message is named by a per-connection counter taken at its head, so the
// delivery half never depends on having seen every earlier frame: frames that
// are dropped between the halves (a generation whose launch failed,
// kmws_rx_batch_discard) leave it consistent.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kmws_gpu.h"
#include "kmws_utf8_rule.hpp"

namespace kmws {

// Bits of a host view above the rule's (bits 0-23 look-back, kUtf8Checked).
constexpr uint32_t kUtf8ViewHead = 1u << 29;        // the frame heads a message (opcode 1-7)
constexpr uint32_t kUtf8ViewFinPending = 1u << 30;  // checked, FIN, and the message ends inside a code point

struct Utf8StreamView {
    uint32_t w = 0;    // look-back | kUtf8Checked | kUtf8ViewHead | kUtf8ViewFinPending
    uint32_t msg = 0;  // the frame's message (counter value at its head); 0: none
};

struct Utf8Stream {
    // parse time
    Utf8Elem state{0u, kUtf8Reset};  // everything fed so far, combined: starts between messages
    uint32_t msg = 0;                // messages begun so far (never 0 for an open one)
    // delivery time
    uint32_t bad_msg = 0;      // the message last reported BAD
    uint32_t dropped_msg = 0;  // the message a dropped generation cut: not checkable any more
};

// kmws_decoder_reset: between messages again.  The counter keeps counting.
inline void utf8_stream_reset(Utf8Stream& s)
{
    s.state = Utf8Elem{0u, kUtf8Reset};
    s.bad_msg = 0;
    s.dropped_msg = 0;
}

// The last nb = min(len, 3) payload bytes, unmasked with `key` (the 4 wire key
// bytes as a little-endian u32; 0 for an unmasked frame), the last in bits 0-7.
inline uint32_t utf8_stream_tail(const uint8_t* payload, size_t len, uint32_t key, uint32_t* nb_out)
{
    const uint32_t nb = len < 3 ? (uint32_t)len : 3u;
    uint32_t tail = 0;
    for (uint32_t k = 0; k < nb; ++k) {
        const size_t j = len - nb + k;
        tail = (tail << 8) | (uint32_t)(payload[j] ^ (uint8_t)(key >> (8u * (j & 3u))));
    }
    *nb_out = nb;
    return tail;
}

// Parse-time half.  op_byte: header byte 0 (fin << 7 | rsv1 << 6 | .. | opcode).
inline Utf8StreamView utf8_stream_frame(Utf8Stream& s, uint32_t op_byte, uint32_t tail, uint32_t nb)
{
    const uint32_t op = op_byte & 0x0Fu;
    const bool head = op >= 1u && op < 8u;
    if (head && ++s.msg == 0u) s.msg = 1u;
    const Utf8View v = utf8_frame_view(s.state, op_byte, 0u);
    Utf8StreamView out;
    out.w = v.w & (0xFFFFFFu | kUtf8Checked);
    if (head) out.w |= kUtf8ViewHead;
    if (out.w & kUtf8Checked) {
        out.msg = s.msg;
        if (op_byte & 0x80u) {  // rule (b): the message's last three bytes = look-back, then this frame's tail
            const Utf8Elem lb{0u, (out.w & 0xFFFFFFu) | (3u << 24)};
            const Utf8Elem tl{0u, (tail & 0xFFFFFFu) | (nb << 24)};
            if (utf8_pending(utf8_elem_ctx(utf8_combine(lb, tl)))) out.w |= kUtf8ViewFinPending;
        }
    }
    s.state = utf8_combine(s.state, utf8_frame_elem(op_byte, 0u, tail, nb));
    return out;
}

// A parsed frame will never be delivered (its generation's launch failed):
// its message, if checked, is no longer checkable -- its later frames, parsed
// already or not, get KMWS_UTF8_NOT_TEXT until the next message head.
inline void utf8_stream_drop(Utf8Stream& s, const Utf8StreamView& v)
{
    if (!(v.w & kUtf8Checked)) return;
    s.dropped_msg = v.msg;
    if (s.msg == v.msg) s.state.w &= ~kUtf8Checked;  // still the open message (or closed: the bit is clear anyway)
}

// Delivery-time half, called in frame order.  dev_bad: the payload pass found a
// byte of this frame that the rule rejects.
inline int utf8_stream_verdict(Utf8Stream& s, const Utf8StreamView& v, bool dev_bad)
{
    if (!(v.w & kUtf8Checked) || v.msg == s.dropped_msg) return KMWS_UTF8_NOT_TEXT;
    if (v.msg == s.bad_msg) return KMWS_UTF8_AFTER_BAD;
    if (dev_bad || (v.w & kUtf8ViewFinPending)) {
        s.bad_msg = v.msg;
        return KMWS_UTF8_BAD;
    }
    return KMWS_UTF8_OK;
}

}  // namespace kmws
