// The protocol state of ONE connection on the host path (kmws_decoder_feed,
// kmws_decoder_feed_deferred / kmws_rx_batch_*): what kmws_proto_check gets from
// its scan over a batch, the host decoder gets from a few instructions per
// frame, because it walks each connection's frames in order anyway.  The state
// is one byte plus the RSV bits the application negotiated.  Host-only, plain
// inline functions over kmws_proto_rule.hpp (the rule is stated there, once);
// tests/cpp/proto_rule_check.cpp drives exactly these.
//
// Unlike the UTF-8 check there is no delivery-time half and no device work:
// the verdict is final when the parser completes the frame.  Only a CLOSE
// frame's payload is looked at, and that is at most 125 bytes, contiguous in
// host memory by then; it is unmasked into a private copy, so the caller's
// bytes are not touched ahead of the payload pass.  A frame that is parsed but
// never delivered still counts: the peer sent it.
// On the decoder's path KMWS_PROTO_HEADER, KMWS_PROTO_CONTROL and
// KMWS_PROTO_AFTER_CLOSE cannot occur: the decoder stops at a header error, at
// a control frame without FIN or above 125 bytes, and after a CLOSE, as kuma
// does (WSHandler.cpp:118-135, :136-156, :265-268).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "kmws_gpu.h"
#include "kmws_proto_rule.hpp"

namespace kmws {

struct ProtoStream {
    uint8_t state = (uint8_t)kProtoIdle;
    uint8_t rsv_allowed = 0;  // of 0x70
};

// kmws_decoder_reset: IDLE again; what was negotiated stays.
inline void proto_stream_reset(ProtoStream& s) { s.state = (uint8_t)kProtoIdle; }

// A completed frame: header byte 0, its payload (len bytes at `payload`, still
// masked with `key`, the 4 wire key bytes as a little-endian u32; 0: plain).
// Returns its KMWS_PROTO_* value and advances the stream.
inline int proto_stream_frame(ProtoStream& s, uint32_t b0, const uint8_t* payload, uint32_t len, uint32_t key)
{
    uint32_t local = proto_local_head(b0, len, 0u, s.rsv_allowed);
    if (local == 0u && proto_needs_body(b0, len)) {  // len <= 125 here: rule 4 passed
        uint8_t body[125];
        for (uint32_t j = 0; j < len; ++j) body[j] = (uint8_t)(payload[j] ^ (uint8_t)(key >> (8u * (j & 3u))));
        local = proto_close_body(body, len, 0u);
    }
    const uint32_t v = proto_verdict(s.state, local, b0);
    s.state = (uint8_t)proto_apply(proto_frame_fn(local, b0), s.state);
    return (int)v;
}

}  // namespace kmws
