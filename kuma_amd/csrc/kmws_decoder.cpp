// WSHandler-compatible streaming decoder of the kmws C ABI
// (src/ws/WSHandler.{h,cpp} in the reference).
//
// The per-byte header state machine stays on the event-loop thread, as in kuma
// (headers arrive byte-serially per connection, WSHandler.cpp:108-280).  The
// payload work -- the reference's scalar unmask loop (WSHandler.cpp:303-310) --
// runs on the GPU, batched:
//   kmws_decoder_feed           one GPU batch per call, callbacks before return
//                               (the drop-in for WSHandler::handleData);
//   kmws_decoder_feed_deferred  frames of many calls / connections staged into
//   + kmws_rx_batch_flush       a kmws_rx_batch; one GPU batch per flush (once
//                               per event-loop iteration), callbacks at flush.
// There is no CPU unmask path: without a usable gfx950 device a masked frame
// fails the call with KMWS_ERR_NOT_SUPPORTED.
// kmws_decoder_set_utf8_check (opt-in): the parser keeps each connection's
// UTF-8 message state (kmws_utf8_stream.hpp), the payload pass validates the
// bytes of checked frames while it unmasks them, and the verdict is delivered
// in kmws_frame_hdr.reserved.  With the check off nothing here changes.
// kmws_decoder_set_proto_check (opt-in): the parser judges each completed frame
// by the sequence and CLOSE rules (kmws_proto_stream.hpp; no GPU), the verdict
// waits with the queued frame and is published on the decoder while the
// frame's callback runs (kmws_decoder_frame_proto).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "kmws_gpu.h"
#include "kmws_host_util.hpp"
#include "kmws_proto_stream.hpp"
#include "kmws_utf8_stream.hpp"

using namespace kmws;

namespace {

enum class St : uint8_t { HDR1, HDR2, HDREX, MASKEY, DATA, CLOSED, IN_ERROR };  // WSHandler.h:57-65

bool is_control(uint8_t op) { return op >= 8; }  // WSHandler.h:52-54

constexpr int kParsing = -100;

// Where a completed frame's payload lives until delivery (synchronous feed).
enum Origin : int {
    kInChunk = 0,        // unmasked (or empty): view into the caller's chunk
    kInChunkPinned = 1,  // masked, caller's chunk is pinned: unmasked there in place by the kernel
    kInChunkStaged = 2,  // masked, pageable chunk: staged, written back in place before delivery
    kStagedMasked = 3,   // masked, reassembled across chunks: view into staging
    kHeld = 4,           // unmasked, reassembled: view into a held reassembly buffer
};

struct Pending {
    kmws_frame_hdr hdr;
    uint8_t* data_ptr;  // in-chunk kinds: payload position in the chunk
    size_t stage_off;   // staged kinds: payload offset in the staging area
    size_t hold_idx;    // kHeld: index into the held buffers
    Origin where;
    Utf8StreamView uv;  // kmws_decoder_set_utf8_check: the frame's view (w == 0: not checked)
    uint32_t slot;      // its verdict byte in the stage (kNoSlot: empty or unchecked, no device work)
    uint8_t proto;      // kmws_decoder_set_proto_check: the frame's KMWS_PROTO_* value (0 with the check off)
};

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

uint32_t op_byte_of(const kmws_frame_hdr& h)
{
    return (uint32_t)((h.fin ? 0x80 : 0) | (h.rsv1 ? 0x40 : 0) | (h.rsv2 ? 0x20 : 0) | (h.rsv3 ? 0x10 : 0) |
                      (h.opcode & 0x0F));
}

}  // namespace

struct kmws_decoder {
    int mode = KMWS_MODE_CLIENT;
    int device = 0;
    bool in_place = true;  // kmws_decoder_set_in_place
    // The last chunk base found pageable: kuma reads into the same buffer every
    // time (TcpConnection.cpp:229), and hipPointerGetAttributes per feed costs
    // more than a small read's unmask.  Only that verdict is remembered: memory
    // pinned since then is still staged (correct, slower), never the reverse.
    const uint8_t* last_pageable = nullptr;
    // DecodeContext (WSHandler.h:66-78)
    kmws_frame_hdr hdr{};
    St state = St::HDR1;
    std::vector<uint8_t> buf;
    uint8_t pos = 0;
    // synchronous-feed delivery lists (the staging is borrowed per call: StagePool)
    std::vector<Pending> pending;
    std::vector<std::vector<uint8_t>> held;
    ExtraBuf chunk;  // the caller's chunk when it is pinned: payloads unmasked where they lie
    // kmws_decoder_set_utf8_check.  The stream's message state, both halves
    // (kmws_utf8_stream.hpp): the parse-time half advances in the feeds' sinks,
    // the delivery-time half (which message was reported BAD) when verdicts are
    // made -- by the synchronous feed before its first callback, by
    // kmws_rx_batch_poll per generation before that generation's first callback
    // and only for items that are still live.
    bool utf8_check = false;
    Utf8Stream utf8;
    // kmws_decoder_set_proto_check.  The state advances in the feeds' sinks
    // (frame_facts); frame_proto holds a frame's verdict while its callback runs.
    bool proto_check = false;
    ProtoStream proto;
    int frame_proto = KMWS_PROTO_OK;

    // What both feeds derive from a completed frame whose payload lies
    // contiguous (and still masked) at `payload`.
    struct Facts {
        bool masked;   // has payload to unmask: handleDataMask is a no-op otherwise (:293, :305)
        bool checked;  // has payload for the UTF-8 check (an empty frame needs no device work: rule (b) is decided here)
        uint32_t key;
        uint32_t dkey;      // its descriptor's key; 0 when unmasked: checked, not stored
        Utf8StreamView uv;  // the frame's view from the parse-time half, which advances here (w == 0: not checked)
        uint8_t proto;      // the frame's KMWS_PROTO_* value; the stream's state advances here too
        bool gpu() const { return masked || checked; }
    };
    Facts frame_facts(const kmws_frame_hdr& h, const uint8_t* payload)
    {
        Facts f{};
        f.masked = h.mask && h.length;
        std::memcpy(&f.key, h.maskey, 4);
        f.dkey = f.masked ? f.key : 0u;
        if (utf8_check) {
            uint32_t nb = 0;
            const uint32_t tail = utf8_stream_tail(payload, h.length, h.mask ? f.key : 0u, &nb);
            f.uv = utf8_stream_frame(utf8, op_byte_of(h), tail, nb);
        }
        f.checked = (f.uv.w & kUtf8Checked) != 0u && h.length;
        if (proto_check)
            f.proto = (uint8_t)proto_stream_frame(proto, op_byte_of(h), payload, h.length, h.mask ? f.key : 0u);
        return f;
    }

    void reset_ctx()  // DecodeContext::reset, WSHandler.h:66-72 (capacity kept)
    {
        std::memset(&hdr, 0, sizeof(hdr));
        state = St::HDR1;
        buf.clear();
        pos = 0;
    }
};

// Stages a batch makes before its first loop iteration (a generation in
// flight each; more are made if needed).
constexpr int kWarmStages = 4;

namespace {

// The generations of an rx or a tx batch: the pinned stage being fed, those of
// the submitted generations with their launches in flight (submit order), the
// finished ones kept for reuse, the stream they all share and the caller's
// attached ring.  Gen: what the batch keeps of a submitted generation beside
// its `stage` member.
template <class Gen>
struct GenQueue {
    BatchStream bstream;  // first: destroyed after every stage that uses it
    std::unique_ptr<PinnedStage> stage;  // the generation being fed
    std::deque<Gen> inflight;
    std::vector<std::unique_ptr<PinnedStage>> spare;
    // The caller's pinned ring (optional), its device view looked up once at
    // attach, and the descriptors of the generation being fed that lie in it.
    ExtraBuf ring;
    int device = 0;

    std::unique_ptr<PinnedStage> take_stage()
    {
        if (!spare.empty()) {
            std::unique_ptr<PinnedStage> s = std::move(spare.back());
            spare.pop_back();
            return s;
        }
        std::unique_ptr<PinnedStage> s(new (std::nothrow) PinnedStage());
        if (s && s->init(device, bstream.s) != KMWS_OK) s.reset();
        return s;
    }
    // the stream, a few warm stages and the first generation's, made before the first loop iteration
    kmws_status prepare(int dev)
    {
        device = dev;
        kmws_status st = bstream.create(dev);
        for (int i = 0; st == KMWS_OK && i < kWarmStages; ++i) {
            std::unique_ptr<PinnedStage> s = take_stage();
            if (!s) return KMWS_ERR_FAILED;
            st = s->warm();
            spare.push_back(std::move(s));
        }
        if (st == KMWS_OK && !(stage = take_stage())) st = KMWS_ERR_FAILED;
        return st;
    }
    // p == nullptr detaches; a ring must be pinned (one of no bytes has no device view)
    kmws_status attach(uint8_t* p, size_t bytes)
    {
        uint8_t* dv = p && bytes ? static_cast<uint8_t*>(device_view(p)) : nullptr;
        if (p && !dv) return KMWS_ERR_INVALID_PARAM;
        ring.base = p;
        ring.dv = dv;
        ring.span = p ? bytes : 0;
        return KMWS_OK;
    }
    // Submitting takes the successor stage first (take_stage(): without one the
    // generation stays as it is), then launches -- a flush (sync) runs one
    // synchronous job on the device's resident worker when it fits one, else
    // launches and waits -- and then either rotates or restores.
    kmws_status launch(bool sync)
    {
        const kmws_status st = sync ? stage->run(ring) : stage->launch(ring, kResMaxBytes);
        ring.list.clear();
        return st;
    }
    // launched: the stage leaves with g, next takes its place
    Gen& rotate(Gen g, std::unique_ptr<PinnedStage> next)
    {
        g.stage = std::move(stage);
        inflight.push_back(std::move(g));
        stage = std::move(next);
        return inflight.back();
    }
    // not launched: the stage stays, emptied
    void restore(std::unique_ptr<PinnedStage> next)
    {
        stage->clear();
        spare.push_back(std::move(next));
    }
    // a finished generation's stage
    void retire(std::unique_ptr<PinnedStage> s)
    {
        s->clear();
        spare.push_back(std::move(s));
    }
    // before the batch is destroyed: no launch may outlive its pinned memory
    void drain()
    {
        for (Gen& g : inflight) (void)g.stage->wait();
    }
};

template <class Batch>
Batch* batch_create(int device)
{
    Batch* b = new (std::nothrow) Batch();
    if (b && b->prepare(resolve_device(device)) != KMWS_OK) {
        delete b;
        b = nullptr;
    }
    return b;
}

template <class Batch>
void batch_destroy(Batch* b)
{
    if (!b) return;
    b->drain();
    delete b;
}

struct RxItem {
    // Identity, and with the UTF-8 check the home of the connection's
    // delivery-time state (Utf8Stream::bad_msg / dropped_msg).  A callback
    // may destroy a decoder, so it is dereferenced in one place only:
    // rx_verdicts / rx_drop_utf8, which run when no callback of the
    // generation has run yet (or none ever will) and touch only items
    // that are still `live` and checked.  That is safe because a decoder may
    // be destroyed only after its frames were delivered or after
    // kmws_rx_batch_discard (the "destroyed" return discards too), and both
    // clear `live` on every item of it -- in the generation being fed, in
    // every generation in flight and in the one being delivered -- before
    // the decoder can be gone.  After kmws_rx_batch_discard the decoder's
    // state is therefore never read or written again through the batch.
    kmws_decoder* dec;
    kmws_frame_cb cb;
    void* user;
    kmws_frame_hdr hdr;
    size_t off;       // payload offset in the generation's staging area (direct == nullptr)
    uint8_t* direct;  // payload in the attached ring (no copy)
    bool live;        // false once discarded
    Utf8StreamView uv;  // the frame's view from the parse-time half (w == 0: not checked)
    uint32_t slot;      // its verdict byte in the generation's stage (kNoSlot: none)
    uint8_t proto;      // the frame's KMWS_PROTO_* value, published on `dec` around its callback (live items only)
};
// One submitted generation: its frames, and the pinned stage that holds
// their staged payloads and the unmask launch in flight.
struct RxGen {
    std::unique_ptr<PinnedStage> stage;
    std::vector<RxItem> items;
};

}  // namespace

struct kmws_rx_batch : GenQueue<RxGen> {
    std::vector<RxItem> items;   // of the generation being fed
    uint64_t pending_bytes = 0;  // masked payload bytes of `items`
    std::vector<RxItem>* delivering = nullptr;  // the generation whose callbacks are running
    bool flushing = false;  // feeding / submitting / polling from inside a delivery is refused
};

namespace {

// Pinned stages for the synchronous entries (kmws_decoder_feed,
// kmws_mask_host_chain), shared by every connection and thread of the process.
// A stage is used only within one call -- its payloads are unmasked and
// delivered before the call returns -- so a call borrows one and gives it back;
// a callback that feeds another decoder borrows another.  The pool holds as
// many stages as calls ever ran at once, each with its stream, event and
// pinned area made once: a decoder per connection (kuma's WSHandler) would
// otherwise create a stream (milliseconds) and 1 MiB of pinned memory per
// connection, and a new loop thread its own.  Never freed (pinned memory must
// not be released after the HIP runtime's teardown at process exit).  Each
// thread keeps the stage it gave back last in front of the pool, so its calls
// take no lock (16 threads masking at once contended on the pool's mutex); a
// nested call, or a call for another device, goes to the pool, and a thread's
// kept stage returns to it when the thread exits.
class StagePool;
StagePool& stage_pool();

// The calling thread's kept stage.  Plain data (zero-initialised, trivially
// destructible), so a call from another thread_local object's destructor after
// the thread's exit hook ran still finds it valid: such a call gives its stage
// to the pool instead of keeping it (which would leak it with the thread).
struct HotStage {
    PinnedStage* s;
    bool gone;  // the thread's exit hook ran
};
thread_local HotStage t_hot;
struct HotStageExit {  // returns the kept stage to the pool at thread exit
    bool armed = false;
    ~HotStageExit();
};
thread_local HotStageExit t_hot_exit;

class StagePool {
public:
    PinnedStage* take(int device, kmws_status* st)
    {
        *st = KMWS_OK;
        if (t_hot.s && t_hot.s->device() == device) {
            PinnedStage* s = t_hot.s;
            t_hot.s = nullptr;
            return s;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t i = free_.size(); i-- > 0;)  // the most recently used first (warm in cache)
                if (free_[i]->device() == device) {
                    PinnedStage* s = free_[i];
                    free_.erase(free_.begin() + (ptrdiff_t)i);
                    return s;
                }
        }
        PinnedStage* s = new (std::nothrow) PinnedStage();
        if (!s) {
            *st = KMWS_ERR_FAILED;
            return nullptr;
        }
        *st = s->init(device);  // KMWS_ERR_NOT_SUPPORTED: no such gfx950 device
        if (*st == KMWS_OK) *st = s->warm();
        if (*st != KMWS_OK) {
            delete s;
            s = nullptr;
        }
        return s;
    }
    void give(PinnedStage* s, bool keep = true)
    {
        s->clear();
        if (keep && !t_hot.s && !t_hot.gone) {
            t_hot_exit.armed = true;  // constructed before the stage is kept: it gives it back
            t_hot.s = s;
            return;
        }
        std::lock_guard<std::mutex> lk(mu_);
        free_.push_back(s);
    }

private:
    std::mutex mu_;
    std::vector<PinnedStage*> free_;
};

StagePool& stage_pool()
{
    static StagePool* p = new StagePool();
    return *p;
}

HotStageExit::~HotStageExit()
{
    t_hot.gone = true;
    if (PinnedStage* s = t_hot.s) {
        t_hot.s = nullptr;
        stage_pool().give(s, false);
    }
}

// A stage borrowed for the scope of one call (taken at first use).
struct BorrowedStage {
    int device;
    PinnedStage* s = nullptr;
    kmws_status st = KMWS_OK;  // why get() failed
    explicit BorrowedStage(int dev) : device(dev) {}
    ~BorrowedStage()
    {
        if (s) stage_pool().give(s);
    }
    PinnedStage* get()
    {
        if (!s) s = stage_pool().take(device, &st);
        return s;
    }
};

// The reference's decodeFrame loop (WSHandler.cpp:108-280).  At every
// completed frame, sink(hdr, payload, reassembly) is called with the payload
// contiguous in memory: in the caller's chunk (reassembly == nullptr) or in
// the decoder's reassembly buffer (the sink may steal it).  Returns the
// WSError of the call, or a negative status the sink returned.
template <class Sink>
int parse_chunk(kmws_decoder* dec, uint8_t* data, size_t len, Sink&& sink)
{
    int result = kParsing;
    size_t p = 0;
    auto& h = dec->hdr;
    while (result == kParsing && p < len) {
        switch (dec->state) {
        case St::HDR1: {  // :118-135
            const uint8_t b = data[p++];
            h.fin = b >> 7;
            h.opcode = b & 0x0F;
            h.rsv1 = (b >> 6) & 1;
            h.rsv2 = (b >> 5) & 1;
            h.rsv3 = (b >> 4) & 1;
            if (!h.fin && is_control(h.opcode)) {
                dec->state = St::IN_ERROR;
                result = KMWS_WS_PROTOCOL_ERROR;
                break;
            }
            dec->state = St::HDR2;
        }
            [[fallthrough]];
        case St::HDR2: {  // :136-156
            if (p >= len) {
                result = KMWS_WS_NEED_MORE_DATA;
                break;
            }
            const uint8_t b = data[p++];
            h.mask = b >> 7;
            h.plen = b & 0x7F;
            h.xpl64 = 0;
            dec->pos = 0;
            dec->buf.clear();
            if (is_control(h.opcode) && h.plen > 125) {
                dec->state = St::IN_ERROR;
                result = KMWS_WS_PROTOCOL_ERROR;
                break;
            }
            dec->state = St::HDREX;
        }
            [[fallthrough]];
        case St::HDREX: {  // :157-204
            if (h.plen == 126) {
                for (; p < len && dec->pos < 2; ++p, ++dec->pos)
                    h.xpl64 = (h.xpl64 & ~0xFFFFull) |
                              (uint16_t)((uint16_t)h.xpl64 | (uint16_t)(data[p] << ((1 - dec->pos) * 8)));
                if (dec->pos < 2) {
                    result = KMWS_WS_NEED_MORE_DATA;
                    break;
                }
                dec->pos = 0;
                if ((uint16_t)h.xpl64 < 126) {
                    dec->state = St::IN_ERROR;
                    result = KMWS_WS_INVALID_LENGTH;
                    break;
                }
                h.length = (uint16_t)h.xpl64;
            } else if (h.plen == 127) {
                // Reference quirk (WSHandler.cpp:179): a promoted 32-bit int
                // shifted by (7-k)*8; x86-64 takes the count mod 32 and the
                // int result is sign-extended into the u64.
                for (; p < len && dec->pos < 8; ++p, ++dec->pos) {
                    const uint32_t sh = ((7u - dec->pos) * 8u) & 31u;
                    h.xpl64 |= (uint64_t)(int64_t)(int32_t)((uint32_t)data[p] << sh);
                }
                if (dec->pos < 8) {
                    result = KMWS_WS_NEED_MORE_DATA;
                    break;
                }
                dec->pos = 0;
                if ((h.xpl64 >> 63) != 0) {
                    dec->state = St::IN_ERROR;
                    result = KMWS_WS_INVALID_LENGTH;
                    break;
                }
                h.length = (uint32_t)h.xpl64;
                if (h.length > KMWS_MAX_FRAME_DATA_LENGTH) {
                    dec->state = St::IN_ERROR;
                    result = KMWS_WS_INVALID_LENGTH;
                    break;
                }
            } else {
                h.length = h.plen;
            }
            dec->state = St::MASKEY;
        }
            [[fallthrough]];
        case St::MASKEY: {  // :205-234
            if (h.mask) {
                if (dec->mode == KMWS_MODE_CLIENT) {
                    dec->state = St::IN_ERROR;
                    result = KMWS_WS_PROTOCOL_ERROR;
                    break;
                }
                size_t c = 4u - dec->pos;
                if (c > len - p) c = len - p;
                std::memcpy(h.maskey + dec->pos, data + p, c);
                p += c;
                dec->pos = (uint8_t)(dec->pos + c);
                if (dec->pos < 4) {
                    result = KMWS_WS_NEED_MORE_DATA;
                    break;
                }
                dec->pos = 0;
            } else if (dec->mode == KMWS_MODE_SERVER && h.length > 0) {
                dec->state = St::IN_ERROR;
                result = KMWS_WS_PROTOCOL_ERROR;
                break;
            }
            dec->buf.clear();
            dec->state = St::DATA;
        }
            [[fallthrough]];
        case St::DATA: {  // :235-272
            if (len - p + dec->buf.size() < h.length) {
                dec->buf.insert(dec->buf.end(), data + p, data + len);
                p = len;
                result = KMWS_WS_NEED_MORE_DATA;
                break;
            }
            int st;
            if (dec->buf.empty()) {  // whole payload in this chunk (:247-250)
                st = sink(h, data + p, (std::vector<uint8_t>*)nullptr);
                p += h.length;
            } else {  // reassembled in ctx_.buf (:251-258)
                const size_t read_len = h.length - dec->buf.size();
                dec->buf.insert(dec->buf.end(), data + p, data + p + read_len);
                p += read_len;
                st = sink(h, dec->buf.data(), &dec->buf);
            }
            if (st != KMWS_OK) return st;
            if (h.opcode == KMWS_OP_CLOSE) {  // :265-268
                dec->state = St::CLOSED;
                result = KMWS_WS_CLOSED;
                break;
            }
            dec->reset_ctx();  // :270
            break;
        }
        default:
            result = KMWS_WS_INVALID_FRAME;  // :273-276
            break;
        }
    }
    if (result == kParsing) result = dec->state == St::HDR1 ? KMWS_WS_NOERR : KMWS_WS_NEED_MORE_DATA;  // :279
    return result;
}

// The descriptor of a frame that goes to the GPU, added to the list of the
// buffer its payload lies in (offset off).  A checked frame takes the next
// verdict byte of the job's stage: returned, else kNoSlot.
uint32_t add_frame_desc(PinnedStage& stage, DescList& list, uint64_t off, uint32_t len, const kmws_decoder::Facts& f)
{
    if (!f.checked) {
        list.add(off, len, f.dkey);
        return kNoSlot;
    }
    const uint32_t slot = stage.utf8_slot();
    list.add_checked(off, len, f.dkey, f.uv.w, slot);
    return slot;
}

}  // namespace

extern "C" {

kmws_decoder* kmws_decoder_create(int mode, int device)
{
    kmws_decoder* d = new (std::nothrow) kmws_decoder();
    if (d) {
        d->mode = mode;
        d->device = resolve_device(device);  // KMWS_DEVICE_AUTO: the creating (loop) thread's GPU
    }
    return d;
}

void kmws_decoder_destroy(kmws_decoder* dec) { delete dec; }

void kmws_decoder_set_mode(kmws_decoder* dec, int mode)
{
    if (dec) dec->mode = mode;
}

void kmws_decoder_reset(kmws_decoder* dec)
{
    if (!dec) return;
    dec->reset_ctx();
    utf8_stream_reset(dec->utf8);  // between messages again
    proto_stream_reset(dec->proto);
}

void kmws_decoder_set_proto_check(kmws_decoder* dec, int on, uint32_t rsv_allowed)
{
    if (!dec) return;
    const bool want = on != 0;
    if (want != dec->proto_check) proto_stream_reset(dec->proto);
    dec->proto_check = want;
    dec->proto.rsv_allowed = (uint8_t)(rsv_allowed & 0x70u);
}

int kmws_decoder_frame_proto(const kmws_decoder* dec) { return dec ? dec->frame_proto : KMWS_PROTO_OK; }

void kmws_decoder_set_utf8_check(kmws_decoder* dec, int on)
{
    if (!dec) return;
    const bool want = on != 0;
    if (want != dec->utf8_check) utf8_stream_reset(dec->utf8);  // switched between messages: nothing is open
    dec->utf8_check = want;
}

// kmws_frame_utf8 as a function, for callers that cannot use the macro (FFI).
#undef kmws_frame_utf8
uint8_t kmws_frame_utf8(const kmws_frame_hdr* h) { return h ? h->reserved : (uint8_t)KMWS_UTF8_NOT_TEXT; }

void kmws_decoder_set_in_place(kmws_decoder* dec, int on)
{
    if (dec) dec->in_place = on != 0;
}

// WSHandler::handleData (WSHandler.cpp:41-44, decodeFrame :108-280) in three
// phases: (1) parse the chunk, collecting completed frames; (2) one GPU unmask
// batch over their masked payloads -- in place in the caller's chunk when it
// is pinned memory, else on a pinned staging copy; (3) deliver in order
// (staged frames that lay in the chunk are first written back there, as the
// reference unmasks them in place), stopping at a callback that destroyed
// the decoder.
int kmws_decoder_feed(kmws_decoder* dec, uint8_t* data, size_t len, kmws_frame_cb cb, void* user)
{
    if (!dec || (len && !data)) return KMWS_ERR_INVALID_PARAM;
    dec->pending.clear();
    dec->held.clear();
    BorrowedStage bs(dec->device);  // given back when the call returns (the decoder may be gone by then)
    int chunk_pinned = -1;  // resolved at the first masked in-chunk frame
    ExtraBuf& chunk = dec->chunk;
    chunk.list.clear();
    chunk.base = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(data) & ~(uintptr_t)15);
    chunk.span = (uint64_t)((data + len) - chunk.base);
    chunk.dv = nullptr;

    auto sink = [&](const kmws_frame_hdr& h, uint8_t* payload, std::vector<uint8_t>* reasm) -> int {
        // A frame with payload that is masked or checked goes to the GPU (key
        // 0 when unmasked: checked, not stored).
        const kmws_decoder::Facts f = dec->frame_facts(h, payload);
        dec->pending.push_back(Pending{h, nullptr, 0, 0, kInChunk, f.uv, kNoSlot, f.proto});
        Pending& qq = dec->pending.back();  // from here on the frame counts as parsed: a failure below drops it
        if (f.gpu() && !bs.get()) return bs.st;
        auto stage_payload = [&]() -> kmws_status {
            const kmws_status st = bs.s->reserve(h.length);
            if (st != KMWS_OK) return st;
            qq.stage_off = bs.s->append(payload, h.length);
            qq.slot = add_frame_desc(*bs.s, bs.s->staged(), qq.stage_off, h.length, f);
            return KMWS_OK;
        };
        if (!reasm) {
            qq.data_ptr = payload;
            if (f.gpu()) {
                if (chunk_pinned < 0) {
                    if (chunk.base != dec->last_pageable) chunk.dv = static_cast<uint8_t*>(device_view(chunk.base));
                    chunk_pinned = chunk.dv != nullptr;
                    if (!chunk_pinned) dec->last_pageable = chunk.base;
                }
                if (chunk_pinned) {
                    qq.slot = add_frame_desc(*bs.s, chunk.list, (uint64_t)(payload - chunk.base), h.length, f);
                    if (f.masked) qq.where = kInChunkPinned;
                } else {
                    const kmws_status st = stage_payload();
                    if (st != KMWS_OK) return st;
                    // an unmasked checked frame is staged for the check only: the view stays on the chunk
                    if (f.masked) qq.where = kInChunkStaged;
                }
            }
        } else if (f.gpu()) {
            const kmws_status st = stage_payload();
            if (st != KMWS_OK) return st;
            qq.where = kStagedMasked;
        } else {
            dec->held.emplace_back();
            dec->held.back().swap(*reasm);
            qq.hold_idx = dec->held.size() - 1;
            qq.where = kHeld;
        }
        return KMWS_OK;
    };

    // The frames parsed by a call that fails are never delivered, but the
    // parse-time half has advanced past them: their open message is no longer
    // checkable until the next message head (utf8_stream_drop).
    auto drop_utf8 = [&] {
        for (const Pending& q : dec->pending) utf8_stream_drop(dec->utf8, q.uv);
    };

    const int result = parse_chunk(dec, data, len, sink);
    if (result < 0) {
        drop_utf8();
        return result;
    }

    // ---- GPU unmask of every masked payload of this call ----
    if (bs.s && (bs.s->n_desc() || !chunk.list.empty())) {
        kmws_status st = bs.s->run(chunk);
        if (st != KMWS_OK) {
            drop_utf8();
            return st;
        }
    }

    // ---- in-order delivery ----
    const bool in_place = dec->in_place;  // the callbacks may destroy the decoder
    // the delivery-time half of the UTF-8 check, for the whole call, while the
    // decoder is certainly alive: hdr.reserved holds the verdict during the callback
    if (dec->utf8_check)
        for (Pending& q : dec->pending)
            q.hdr.reserved = (uint8_t)utf8_stream_verdict(dec->utf8, q.uv, q.slot != kNoSlot && bs.s->utf8_bad(q.slot));
    std::vector<Pending> todo;
    todo.swap(dec->pending);
    std::vector<std::vector<uint8_t>> held;
    held.swap(dec->held);
    uint8_t* stage = bs.s ? bs.s->data() : nullptr;
    for (Pending& q : todo) {
        uint8_t* payload;
        switch (q.where) {
        case kInChunkStaged:  // unmasked in place in the caller's buffer, as kuma does (:260)
            if (!in_place) {     // or the view points at the unmasked staging copy
                payload = stage + q.stage_off;
                break;
            }
            std::memcpy(q.data_ptr, stage + q.stage_off, q.hdr.length);
            payload = q.data_ptr;
            break;
        case kStagedMasked: payload = stage + q.stage_off; break;
        case kHeld: payload = held[q.hold_idx].data(); break;
        default: payload = q.data_ptr; break;  // kInChunk, kInChunkPinned
        }
        // WSHandler::handleFrame (:282-289): a callback that destroyed its
        // owner ends the call; the decoder must not be touched afterwards.
        // the decoder is alive until a callback says otherwise: the verdict is
        // published for the callback and cleared behind it
        dec->frame_proto = q.proto;
        if (cb && cb(&q.hdr, payload, q.hdr.length, user)) return KMWS_WS_DESTROYED;
        dec->frame_proto = KMWS_PROTO_OK;
    }
    return result;
}

// ---- host-buffer masking: WSHandler::handleDataMask statics (a-1, a-2) ----

// Masks a chain of host segments in place with the key phase continuing across
// segments (WSHandler.cpp:312-322; one segment = :303-310).  The segments are
// gathered back to back into pinned staging -- so the chain is one payload and
// one descriptor -- unmasked by the GPU in place there, and scattered back.
kmws_status kmws_mask_host_chain(const uint8_t key[KMWS_MASK_KEY_SIZE], uint8_t* const* segs, const size_t* lens,
                                 size_t nseg, int device)
{
    if (!key || (nseg && (!segs || !lens))) return KMWS_ERR_INVALID_PARAM;
    size_t total = 0;
    for (size_t i = 0; i < nseg; ++i) {
        if (lens[i] && !segs[i]) return KMWS_ERR_INVALID_PARAM;
        total += lens[i];
    }
    if (total == 0) return KMWS_OK;  // nothing to do (:305)
    if (total > 0xFFFFFFFFull) return KMWS_ERR_INVALID_PARAM;
    if (device == KMWS_DEVICE_AUTO) {
        device = kmws_thread_device();
        if (device < 0) return device;
    }
    if (device < 0) return KMWS_ERR_INVALID_PARAM;
    BorrowedStage bs(device);  // a stage of the process's pool for this call (StagePool)
    PinnedStage* s = bs.get();
    if (!s) return bs.st;
    kmws_status st = s->reserve(total);
    if (st != KMWS_OK) return st;
    size_t off = 0;
    uint8_t* dst = s->alloc(total, &off);
    size_t pos = 0;
    for (size_t i = 0; i < nseg; ++i) {
        if (lens[i]) std::memcpy(dst + pos, segs[i], lens[i]);
        pos += lens[i];
    }
    uint32_t k;
    std::memcpy(&k, key, 4);
    s->staged().add(off, (uint32_t)total, k);
    st = s->run();
    if (st != KMWS_OK) return st;
    pos = 0;
    for (size_t i = 0; i < nseg; ++i) {
        if (lens[i]) std::memcpy(segs[i], dst + pos, lens[i]);
        pos += lens[i];
    }
    return KMWS_OK;
}

// ---- pinned host rings ----

void* kmws_host_alloc(size_t bytes, int device)
{
    device = resolve_device(device);
    if (bytes == 0 || device < 0 || kmws_device_count() <= device) return nullptr;
    DevGuard g(device);
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

void kmws_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

// ---- batched send path (SURVEY f-2) ----
//
// Sends queued with kmws_tx_batch_add form the current generation;
// kmws_tx_batch_submit enqueues ONE mask launch for it and returns a ticket;
// kmws_tx_batch_poll(ticket) completes generations up to the ticket (staged
// segments are copied back into the caller's buffers) -- the loop writes a
// generation's iovecs once its ticket completed, and can fill and submit the
// next generation meanwhile.  kmws_tx_batch_flush = submit + poll(wait).

struct TxSeg {
    uint8_t* p;
    size_t len;
};
struct TxFrame {
    size_t seg0, nseg;  // range in segs
    size_t bytes;
    uint32_t key;
};
struct TxGen {  // submitted: the stage with the launch in flight, segments to copy back
    std::unique_ptr<PinnedStage> stage;
    std::vector<TxSeg> segs;
    std::vector<size_t> offs;  // staging offset per segment (SIZE_MAX: masked in the ring)
    int64_t ticket;
};

struct kmws_tx_batch : GenQueue<TxGen> {
    std::vector<TxSeg> segs;
    std::vector<TxFrame> frames;
    size_t bytes = 0;
    int64_t next_ticket = 1, done_ticket = 0;
};

kmws_tx_batch* kmws_tx_batch_create(int device) { return batch_create<kmws_tx_batch>(device); }

void kmws_tx_batch_destroy(kmws_tx_batch* b) { batch_destroy(b); }

int kmws_tx_batch_pending(const kmws_tx_batch* b) { return b ? (int)b->frames.size() : 0; }

// sendWsFrame (WebSocketImpl.cpp:405-436) up to the socket write: length =
// u32(chain length) (:415), header packed (:416), payload queued for masking
// when the header says so and it is not empty (:410-414); more than 128
// non-empty segments -> BUFFER_TOO_LONG after the mask, as kuma (:419-431).
int kmws_tx_batch_add(kmws_tx_batch* b, const kmws_frame_hdr* hdr, uint8_t* const* segs, const size_t* lens,
                      size_t nseg, uint8_t hdr_out[KMWS_MAX_HEADER_SIZE])
{
    if (!b || !hdr || !hdr_out || (nseg && (!segs || !lens))) return KMWS_ERR_INVALID_PARAM;
    size_t plen = 0, nonempty = 0;
    for (size_t i = 0; i < nseg; ++i) {
        if (lens[i] && !segs[i]) return KMWS_ERR_INVALID_PARAM;
        plen += lens[i];
        nonempty += lens[i] != 0;
    }
    if (plen > 0xFFFFFFFFull) return KMWS_ERR_INVALID_PARAM;
    kmws_frame_hdr h = *hdr;
    h.length = (uint32_t)plen;
    const int hl = kmws_encode_header(&h, hdr_out);
    if (h.mask && plen > 0) {
        uint32_t key;
        std::memcpy(&key, h.maskey, 4);
        b->frames.push_back(TxFrame{b->segs.size(), 0, plen, key});
        for (size_t i = 0; i < nseg; ++i)
            if (lens[i]) b->segs.push_back(TxSeg{segs[i], lens[i]});
        b->frames.back().nseg = b->segs.size() - b->frames.back().seg0;
        b->bytes += plen;
    }
    return 1 + nonempty > 129 ? KMWS_ERR_BUFFER_TOO_LONG : hl;
}

// kmws_tx_batch_attach_ring: segments inside it are masked there (zero-copy).
kmws_status kmws_tx_batch_attach_ring(kmws_tx_batch* b, uint8_t* ring, size_t ring_bytes)
{
    if (!b || (ring && !ring_bytes)) return KMWS_ERR_INVALID_PARAM;
    // queued segments were classified already; a mask in flight may still be writing into the old ring
    if (!b->frames.empty() || !b->inflight.empty()) return KMWS_ERR_INVALID_STATE;
    return b->attach(ring, ring_bytes);
}

// One descriptor per segment, its key rotated by the frame bytes before it
// (the phase continues across segments, WSHandler.cpp:312-322): segments in
// the attached pinned ring are masked in place there, the others gathered
// into pinned staging and copied back when the generation completes; one
// launch per buffer -- or, for a flush (sync), one synchronous job on the
// device's resident worker (kmws_resident.hip) when it fits one.
static int64_t tx_submit(kmws_tx_batch* b, bool sync)
{
    if (!b) return KMWS_ERR_INVALID_PARAM;
    if (b->frames.empty()) return 0;
    std::unique_ptr<PinnedStage> next = b->take_stage();
    if (!next) return KMWS_ERR_FAILED;
    PinnedStage& s = *b->stage;
    s.clear();  // the generation is staged here, not at kmws_tx_batch_add
    b->ring.list.clear();
    size_t staged = 0;
    for (const TxSeg& g : b->segs)
        if (!b->ring.holds(g.p, g.len)) staged += g.len + 16;
    kmws_status st = s.reserve(staged);
    std::vector<size_t> offs(b->segs.size(), SIZE_MAX);
    if (st == KMWS_OK) {
        for (const TxFrame& fr : b->frames) {
            size_t phase = 0;
            for (size_t i = fr.seg0; i < fr.seg0 + fr.nseg; ++i) {
                const TxSeg& g = b->segs[i];
                const uint32_t key = __builtin_rotateright32(fr.key, 8u * (uint32_t)(phase & 3u));
                if (b->ring.holds(g.p, g.len)) {
                    b->ring.list.add((uint64_t)(g.p - b->ring.base), (uint32_t)g.len, key);
                } else {
                    uint8_t* dst = s.alloc(g.len, &offs[i]);
                    std::memcpy(dst, g.p, g.len);
                    s.staged().add(offs[i], (uint32_t)g.len, key);
                }
                phase += g.len;
            }
        }
        st = b->launch(sync);
    }
    b->frames.clear();
    b->bytes = 0;
    if (st != KMWS_OK) {
        b->segs.clear();
        b->restore(std::move(next));
        return st;
    }
    TxGen g;
    g.segs.swap(b->segs);
    g.offs.swap(offs);
    g.ticket = b->next_ticket++;
    return b->rotate(std::move(g), std::move(next)).ticket;
}

int64_t kmws_tx_batch_submit(kmws_tx_batch* b) { return tx_submit(b, false); }

int kmws_tx_batch_poll(kmws_tx_batch* b, int64_t ticket, int wait)
{
    if (!b || ticket < 0) return KMWS_ERR_INVALID_PARAM;
    kmws_status err = KMWS_OK;
    while (!b->inflight.empty() && b->inflight.front().ticket <= ticket) {
        TxGen& g = b->inflight.front();
        if (!wait && !g.stage->done()) break;
        const kmws_status st = g.stage->wait();
        if (st == KMWS_OK) {
            for (size_t i = 0; i < g.segs.size(); ++i)
                if (g.offs[i] != SIZE_MAX) std::memcpy(g.segs[i].p, g.stage->data() + g.offs[i], g.segs[i].len);
        } else {
            err = st;
        }
        b->done_ticket = g.ticket;
        b->retire(std::move(g.stage));
        b->inflight.pop_front();
    }
    if (err != KMWS_OK) return err;
    return ticket <= b->done_ticket || b->inflight.empty() || b->inflight.front().ticket > ticket ? 1 : 0;
}

int64_t kmws_tx_batch_flush(kmws_tx_batch* b)
{
    if (!b) return KMWS_ERR_INVALID_PARAM;
    const int64_t nf = (int64_t)b->frames.size();
    // what is in flight first: the thread's resident slot holds one job, and a
    // job posted while the previous one runs launches instead
    if (!b->inflight.empty()) {
        const int r0 = kmws_tx_batch_poll(b, b->next_ticket - 1, 1);
        if (r0 < 0) return r0;
    }
    const int64_t t = tx_submit(b, true);  // masked when it returns: the poll only copies back
    if (t < 0) return t;
    const int r = kmws_tx_batch_poll(b, b->next_ticket - 1, 1);
    if (r < 0) return r;
    return nf;
}

// ---- deferred delivery across calls and connections ----
//
// Frames fed with kmws_decoder_feed_deferred collect in the batch's current
// generation (payloads copied into its pinned stage, or left where they lie in
// the attached ring).  kmws_rx_batch_submit enqueues ONE unmask launch for the
// generation and returns at once; kmws_rx_batch_poll delivers the callbacks of
// every generation whose launch has finished, in submit order (wait != 0: all
// of them).  kmws_rx_batch_flush = submit + poll(wait).  So an event loop can
// submit at the end of an iteration and deliver at the next one: the GPU round
// trip overlaps the loop's socket reads instead of stalling them.

kmws_rx_batch* kmws_rx_batch_create(int device) { return batch_create<kmws_rx_batch>(device); }

void kmws_rx_batch_destroy(kmws_rx_batch* b) { batch_destroy(b); }

int kmws_decoder_feed_deferred(kmws_decoder* dec, kmws_rx_batch* b, const uint8_t* data, size_t len,
                               kmws_frame_cb cb, void* user)
{
    if (!dec || !b || (len && !data)) return KMWS_ERR_INVALID_PARAM;
    if (b->flushing) return KMWS_ERR_INVALID_STATE;
    // The chunk does not outlive this call (kuma reads into a stack buffer,
    // TcpConnection.cpp:229), so every payload is copied into the batch unless
    // it lies in the attached ring.  The parse does not write into the chunk.
    auto sink = [&](const kmws_frame_hdr& h, uint8_t* payload, std::vector<uint8_t>* reasm) -> int {
        // a frame with payload that is masked or checked gets a descriptor
        // (key 0 when unmasked: checked, not stored)
        const kmws_decoder::Facts f = dec->frame_facts(h, payload);
        if (f.masked) b->pending_bytes += h.length;
        // queued first: a frame the parse-time half has seen must be dropped
        // through rx_drop_utf8 if its payload cannot be staged
        b->items.push_back(RxItem{dec, cb, user, h, 0, nullptr, true, f.uv, kNoSlot, f.proto});
        RxItem& it = b->items.back();
        if (!reasm && b->ring.holds(payload, h.length)) {
            // payload lies in the caller's pinned ring: unmasked there, no copy
            it.direct = payload;
            const uint64_t off = (uint64_t)(payload - b->ring.base);
            if (f.gpu()) it.slot = add_frame_desc(*b->stage, b->ring.list, off, h.length, f);
            return KMWS_OK;
        }
        const kmws_status st = b->stage->reserve(h.length);
        if (st != KMWS_OK) {
            utf8_stream_drop(dec->utf8, f.uv);
            b->items.pop_back();
            return st;
        }
        it.off = b->stage->append(payload, h.length);
        if (f.gpu()) it.slot = add_frame_desc(*b->stage, b->stage->staged(), it.off, h.length, f);
        return KMWS_OK;
    };
    return parse_chunk(dec, const_cast<uint8_t*>(data), len, sink);
}

// The frames of a generation that will never be delivered (its launch failed):
// the parse-time half of their decoders has advanced past them, so their open
// messages are no longer checkable until the next message head.  Live items
// only: a discarded item's decoder may be gone (see RxItem::dec).
static void rx_drop_utf8(std::vector<RxItem>& items)
{
    for (auto& it : items)
        if (it.live && (it.uv.w & kUtf8Checked)) utf8_stream_drop(it.dec->utf8, it.uv);
}

// The delivery-time half for a whole generation, before its first callback:
// hdr.reserved holds the verdict while the frame's callback runs.
static void rx_verdicts(std::vector<RxItem>& items, const PinnedStage& stage)
{
    for (auto& it : items)
        if (it.live && (it.uv.w & kUtf8Checked))
            it.hdr.reserved =
                (uint8_t)utf8_stream_verdict(it.dec->utf8, it.uv, it.slot != kNoSlot && stage.utf8_bad(it.slot));
}

kmws_status kmws_rx_batch_attach_ring(kmws_rx_batch* b, uint8_t* ring, size_t bytes)
{
    if (!b || b->flushing || !b->items.empty() || !b->inflight.empty()) return KMWS_ERR_INVALID_STATE;
    return b->attach(ring, bytes);
}

int kmws_rx_batch_pending(const kmws_rx_batch* b) { return b ? (int)b->items.size() : 0; }

uint64_t kmws_rx_batch_pending_bytes(const kmws_rx_batch* b) { return b ? b->pending_bytes : 0; }

int kmws_rx_batch_inflight(const kmws_rx_batch* b) { return b ? (int)b->inflight.size() : 0; }

void kmws_rx_batch_discard(kmws_rx_batch* b, const kmws_decoder* dec)
{
    if (!b) return;
    for (auto& it : b->items)
        if (it.dec == dec) it.live = false;
    for (auto& g : b->inflight)
        for (auto& it : g.items)
            if (it.dec == dec) it.live = false;
    if (b->delivering)
        for (auto& it : *b->delivering)
            if (it.dec == dec) it.live = false;
}

// sync (a flush): one synchronous job on the device's resident worker when it
// fits one (else a launch and a wait), instead of an enqueued launch.
static int rx_submit(kmws_rx_batch* b, bool sync)
{
    if (!b) return KMWS_ERR_INVALID_PARAM;
    if (b->flushing) return KMWS_ERR_INVALID_STATE;
    if (b->items.empty()) return 0;
    std::unique_ptr<PinnedStage> next = b->take_stage();
    if (!next) return KMWS_ERR_FAILED;
    const kmws_status st = b->launch(sync);  // the payloads were staged at feed time
    b->pending_bytes = 0;
    if (st != KMWS_OK) {
        // nothing of this generation can be delivered masked: drop it
        rx_drop_utf8(b->items);
        b->items.clear();
        b->restore(std::move(next));
        return st;
    }
    const int n = (int)b->items.size();
    RxGen g;
    g.items.swap(b->items);
    b->rotate(std::move(g), std::move(next));
    return n;
}

int kmws_rx_batch_submit(kmws_rx_batch* b) { return rx_submit(b, false); }

int kmws_rx_batch_poll(kmws_rx_batch* b, int wait)
{
    if (!b) return KMWS_ERR_INVALID_PARAM;
    if (b->flushing) return KMWS_ERR_INVALID_STATE;
    int delivered = 0;
    kmws_status err = KMWS_OK;
    while (!b->inflight.empty()) {
        RxGen& g = b->inflight.front();
        if (!wait && !g.stage->done()) break;
        const kmws_status st = g.stage->wait();
        std::vector<RxItem> items;
        items.swap(g.items);
        std::unique_ptr<PinnedStage> stage = std::move(g.stage);
        b->inflight.pop_front();
        if (st != KMWS_OK) {  // the launch failed: these payloads are still masked, never delivered
            err = st;
            rx_drop_utf8(items);
            b->retire(std::move(stage));
            continue;
        }
        rx_verdicts(items, *stage);  // before the first callback: every live item's decoder is alive
        b->flushing = true;
        b->delivering = &items;
        for (auto& it : items) {
            if (!it.live) continue;
            ++delivered;  // a NULL callback consumes the frame, like WSHandler without frame_cb_ (:286)
            uint8_t* payload = it.direct ? it.direct : stage->data() + it.off;
            // "destroyed" (WSHandler.cpp:284-287): none of that decoder's frames
            // may reach its callback again -- the rest of this generation, every
            // later generation in flight and the one still being fed
            // a live item's decoder is alive (see RxItem::dec); after the callback
            // it is touched again only if the item is still live
            it.dec->frame_proto = it.proto;
            if (it.cb && it.cb(&it.hdr, payload, it.hdr.length, it.user)) kmws_rx_batch_discard(b, it.dec);
            if (it.live) it.dec->frame_proto = KMWS_PROTO_OK;
        }
        b->delivering = nullptr;
        b->flushing = false;
        b->retire(std::move(stage));
    }
    return err != KMWS_OK ? err : delivered;
}

int kmws_rx_batch_flush(kmws_rx_batch* b)
{
    // the generations in flight first (delivered in order, before this one):
    // the thread's resident slot holds one job, and a job posted while the
    // previous one runs launches instead (the loopback's ring-wrap flushes did)
    int d0 = 0;
    if (b && !b->flushing && !b->inflight.empty()) {
        d0 = kmws_rx_batch_poll(b, 1);
        if (d0 < 0) return d0;
    }
    const int s = rx_submit(b, true);
    const int d = kmws_rx_batch_poll(b, 1);
    return s < 0 ? s : d < 0 ? d : d0 + d;
}

}  // extern "C"
