/*
 * ref_wrap.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * extern "C" wrapper that puts the oracle's ABI (oracle/kmws_oracle.c), under
 * a ref_ prefix, in front of the reference's own compiled WSHandler.cpp.
 * oracle/ref_build.py compiles the two together into
 * oracle/_ref/libkmws_ref_O3.so and libkmws_ref_O0.so; neither those libraries
 * nor any reference text is committed.  The product never loads them.
 *
 * There is no ref_decoder_state: WSHandler has no accessor for its decode
 * state and this wrapper does not pry private members open.
 */
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "WSHandler.h"

using kuma::KMBuffer;
using kuma::KMError;
using kuma::ws::FrameHeader;
using kuma::ws::WSError;
using kuma::ws::WSHandler;
using kuma::ws::WSMode;

extern "C" {

/* Same layout as orc_hdr in kmws_oracle.c. */
typedef struct orc_hdr {
    uint8_t fin, rsv1, rsv2, rsv3, opcode, mask, plen, _pad;
    uint64_t xpl64;
    uint8_t maskey[4];
    uint32_t length;
} orc_hdr;

typedef int (*orc_frame_cb)(const orc_hdr* hdr, const uint8_t* payload, size_t len, void* user);

} // extern "C"

namespace {

struct RefDecoder {
    WSHandler* handler = nullptr;   /* nullptr once a callback has destroyed it */
    orc_frame_cb cb = nullptr;      /* valid for the duration of one feed */
    void* user = nullptr;
};

void install_callback(RefDecoder* d)
{
    d->handler->setFrameCallback([d](FrameHeader fh, KMBuffer& buf) -> KMError {
        RefDecoder* self = d;       /* the closure dies with the handler below */
        orc_hdr h;
        memset(&h, 0, sizeof(h));
        h.fin = fh.fin; h.rsv1 = fh.rsv1; h.rsv2 = fh.rsv2; h.rsv3 = fh.rsv3;
        h.opcode = fh.opcode; h.mask = fh.mask; h.plen = fh.plen;
        h.xpl64 = fh.xpl.xpl64;
        memcpy(h.maskey, fh.maskey, 4);
        h.length = fh.length;
        if (self->cb && self->cb(&h, static_cast<const uint8_t*>(buf.readPtr()), buf.length(), self->user)) {
            /* "the callback destroyed the handler": really delete it, inside
             * its own callback, so that handleFrame's destroy check is what
             * ends the feed. */
            WSHandler* dead = self->handler;
            self->handler = nullptr;
            delete dead;
        }
        return KMError::NOERR;
    });
}

} // namespace

extern "C" {

/* Phase 0: the flat handleDataMask(key, data, len).  Phase != 0: the
 * KMBuffer-chain overload over a chain whose first segment holds `phase`
 * scratch bytes and whose second is `data`. */
void ref_mask(const uint8_t key[4], uint8_t* data, size_t len, size_t phase)
{
    if (phase == 0) {
        WSHandler::handleDataMask(key, data, len);
        return;
    }
    std::vector<uint8_t> lead(phase);
    KMBuffer head(lead.data(), phase, phase);
    KMBuffer body(data, len, len);
    head.append(&body);
    WSHandler::handleDataMask(key, head);
}

/* The chain overload over n caller segments (empty ones included), in place. */
void ref_mask_chain(const uint8_t key[4], uint8_t* const* segs, const size_t* lens, size_t n)
{
    if (n == 0) return;
    std::vector<std::unique_ptr<KMBuffer>> bufs;
    for (size_t i = 0; i < n; ++i) {
        bufs.emplace_back(new KMBuffer(static_cast<void*>(segs[i]), lens[i], lens[i]));
        if (i) bufs[0]->append(bufs[i].get());
    }
    WSHandler::handleDataMask(key, *bufs[0]);
}

int ref_encode_header(const orc_hdr* h, uint8_t out[WS_MAX_HEADER_SIZE])
{
    FrameHeader fh;
    memset(&fh, 0, sizeof(fh));
    fh.fin = h->fin; fh.rsv1 = h->rsv1; fh.rsv2 = h->rsv2; fh.rsv3 = h->rsv3;
    fh.opcode = h->opcode; fh.mask = h->mask; fh.plen = h->plen;
    fh.xpl.xpl64 = h->xpl64;
    memcpy(fh.maskey, h->maskey, 4);
    fh.length = h->length;
    return WSHandler::encodeFrameHeader(fh, out);
}

/* WSHandler's constructor leaves ctx_.hdr indeterminate until the first
 * reset() (its only initialised member is `length`), and a frame's callback
 * passes hdr.maskey through even when the frame is unmasked.  One reset()
 * straight after construction makes every observable defined, so that no test
 * reads indeterminate memory; it changes nothing else (state, buf and pos
 * already have their reset values). */
void* ref_decoder_create(int mode)
{
    RefDecoder* d = new RefDecoder;
    d->handler = new WSHandler;
    d->handler->setMode(mode ? WSMode::SERVER : WSMode::CLIENT);
    d->handler->reset();
    install_callback(d);
    return d;
}

void ref_decoder_destroy(void* p)
{
    RefDecoder* d = static_cast<RefDecoder*>(p);
    if (!d) return;
    delete d->handler;
    delete d;
}

void ref_decoder_reset(void* p)
{
    RefDecoder* d = static_cast<RefDecoder*>(p);
    if (d->handler) d->handler->reset();
}

void ref_decoder_set_mode(void* p, int mode)
{
    RefDecoder* d = static_cast<RefDecoder*>(p);
    if (d->handler) d->handler->setMode(mode ? WSMode::SERVER : WSMode::CLIENT);
}

int ref_decoder_feed(void* p, uint8_t* data, size_t len, orc_frame_cb cb, void* user)
{
    RefDecoder* d = static_cast<RefDecoder*>(p);
    if (!d->handler) return static_cast<int>(WSError::DESTROYED);
    d->cb = cb;
    d->user = user;
    int ret = static_cast<int>(d->handler->handleData(data, len));
    d->cb = nullptr;
    d->user = nullptr;
    return ret;
}

} // extern "C"
