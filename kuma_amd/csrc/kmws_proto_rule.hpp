// RFC 6455 frame-sequence and CLOSE rules of one stream, stated once for the
// host decoder (kmws_proto_stream.hpp) and the device scan (kmws_proto.hip).
// Plain __host__ __device__ functions: tests/cpp/proto_rule_check.cpp runs the
// very functions the kernels call.
//
// A stream is IDLE (between messages), OPEN (a data message is unfinished),
// CLOSED (a valid CLOSE was seen) or FAILED.  Frame i is b0 = header byte 0
// (fin << 7 | rsv << 4 | opcode), its payload length, the parser's error byte if
// there is one and, for a CLOSE frame only, its payload.
//
// Local class of a frame -- what is wrong with it whatever came before; the
// first rule that matches decides:
//   1. the parser reported a header error                          -> HEADER
//   2. an RSV bit that is not allowed: on a data head (opcode 1, 2) the bits
//      the caller negotiated (RFC 7692 6 for RSV1), none on CONTINUE or on a
//      control frame                                                -> RSV
//   3. opcode 3..7 or 11..15 (5.2: reserved)                        -> OPCODE
//   4. a control frame without FIN or longer than 125 bytes (5.5)   -> CONTROL
//   5. CLOSE (5.5.1, 7.4): one payload byte, or a status code outside
//      {1000-1003, 1007-1014, 3000-4999}                            -> CLOSE_PAYLOAD
//      else a reason [2, len) that is not a complete well-formed UTF-8
//      string (kmws_utf8_rule.hpp)                                  -> CLOSE_REASON
//   6. else 0.
// Verdict and next state, given the state before the frame:
//   FAILED: AFTER_FAIL, stays.  CLOSED: AFTER_CLOSE, stays.
//   a nonzero local class: that class, FAILED.
//   IDLE and CONTINUE: CONTINUATION, FAILED.  OPEN and opcode 1 / 2: INTERLEAVED, FAILED.
//   anything else: OK; CLOSE -> CLOSED, PING / PONG -> unchanged, a data frame
//   -> IDLE with FIN, else OPEN.
//
// What a frame does to the state is a function {4 states} -> {4 states}: one
// byte, two bits per input state (bits 2s, 2s + 1 = the state after, from s).
// Functions compose associatively, so the state before every frame of a batch
// is a scan; a stream's first frame is composed behind the constant function of
// its carried state, which absorbs everything in front of it -- no reset flag.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "kmws_gpu.h"
#include "kmws_utf8_rule.hpp"

namespace kmws {

constexpr uint32_t kProtoIdle = 0, kProtoOpen = 1, kProtoClosed = 2, kProtoFailed = 3;

// kScanBlockFrames (kmws_stream_scan.hpp; kmws_proto.hip ties them), exported for the tests, which read this line.
constexpr uint32_t kProtoBlockFrames = 1024;

KMWS_HD uint32_t proto_identity() { return 0xE4u; }                   // 3, 2, 1, 0 -> themselves
KMWS_HD uint32_t proto_const(uint32_t state) { return (state & 3u) * 0x55u; }
KMWS_HD uint32_t proto_apply(uint32_t f, uint32_t state) { return (f >> (2u * (state & 3u))) & 3u; }
// a, then b
KMWS_HD uint32_t proto_compose(uint32_t a, uint32_t b)
{
    return proto_apply(b, a) | (proto_apply(b, a >> 2) << 2) | (proto_apply(b, a >> 4) << 4) |
           (proto_apply(b, a >> 6) << 6);
}
KMWS_HD uint32_t proto_fn(uint32_t from_idle, uint32_t from_open)
{
    return from_idle | (from_open << 2) | (kProtoClosed << 4) | (kProtoFailed << 6);
}

// The state function of a frame with local class `local` and header byte 0 b0.
KMWS_HD uint32_t proto_frame_fn(uint32_t local, uint32_t b0)
{
    const uint32_t op = b0 & 15u, after_data = (b0 & 0x80u) ? kProtoIdle : kProtoOpen;
    if (local != 0u) return proto_fn(kProtoFailed, kProtoFailed);
    if (op == KMWS_OP_CLOSE) return proto_fn(kProtoClosed, kProtoClosed);
    if (op >= 8u) return proto_identity();
    if (op == 0u) return proto_fn(kProtoFailed, after_data);
    return proto_fn(after_data, kProtoFailed);
}

// The KMWS_PROTO_* value of that frame, the stream being in `state` before it.
KMWS_HD uint32_t proto_verdict(uint32_t state, uint32_t local, uint32_t b0)
{
    const uint32_t op = b0 & 15u;
    if (state == kProtoFailed) return KMWS_PROTO_AFTER_FAIL;
    if (state == kProtoClosed) return KMWS_PROTO_AFTER_CLOSE;
    if (local != 0u) return local;
    if (state == kProtoIdle && op == 0u) return KMWS_PROTO_CONTINUATION;
    if (state == kProtoOpen && (op == 1u || op == 2u)) return KMWS_PROTO_INTERLEAVED;
    return KMWS_PROTO_OK;
}

// Rules 1-4 and the one-byte CLOSE: everything that needs no payload byte.
KMWS_HD uint32_t proto_local_head(uint32_t b0, uint32_t len, uint32_t err, uint32_t rsv_allowed)
{
    const uint32_t op = b0 & 15u, rsv = b0 & 0x70u;
    if (err != 0u) return KMWS_PROTO_HEADER;
    if (rsv & ~((op == 1u || op == 2u) ? rsv_allowed : 0u)) return KMWS_PROTO_RSV;
    if ((op >= 3u && op <= 7u) || op >= 11u) return KMWS_PROTO_OPCODE;
    if (op >= 8u && (!(b0 & 0x80u) || len > 125u)) return KMWS_PROTO_CONTROL;
    if (op == KMWS_OP_CLOSE && len == 1u) return KMWS_PROTO_CLOSE_PAYLOAD;
    return 0u;
}
// A frame whose class is still 0 after proto_local_head and whose payload decides (rule 5).
KMWS_HD bool proto_needs_body(uint32_t b0, uint32_t len) { return (b0 & 15u) == KMWS_OP_CLOSE && len >= 2u; }

KMWS_HD bool proto_close_code_ok(uint32_t code)
{
    return (code >= 1000u && code <= 1003u) || (code >= 1007u && code <= 1014u) || (code >= 3000u && code <= 4999u);
}
// Rule 5 on the len (2..125) payload bytes at p, still masked with `key` (the 4
// wire key bytes as a little-endian u32; 0: plain).  A serial walk of at most
// 123 reason bytes.
KMWS_HD uint32_t proto_close_body(const uint8_t* p, uint32_t len, uint32_t key)
{
    const uint32_t c0 = p[0] ^ (key & 0xFFu), c1 = p[1] ^ ((key >> 8) & 0xFFu);
    if (!proto_close_code_ok((c0 << 8) | c1)) return KMWS_PROTO_CLOSE_PAYLOAD;
    uint32_t L = 0;
    bool bad = false;
    for (uint32_t j = 2; j < len; ++j) {
        const uint32_t b = p[j] ^ ((key >> (8u * (j & 3u))) & 0xFFu);
        bad |= utf8_byte_bad(b, L);
        L = utf8_append(L, b);
    }
    return (bad || utf8_pending(L)) ? (uint32_t)KMWS_PROTO_CLOSE_REASON : 0u;
}

// The whole local class; payload is read only for a CLOSE frame that rules 1-4 pass.
KMWS_HD uint32_t proto_local(uint32_t b0, uint32_t len, uint32_t err, uint32_t rsv_allowed, const uint8_t* payload,
                             uint32_t key)
{
    const uint32_t head = proto_local_head(b0, len, err, rsv_allowed);
    if (head != 0u || !proto_needs_body(b0, len)) return head;
    return proto_close_body(payload, len, key);
}

}  // namespace kmws
