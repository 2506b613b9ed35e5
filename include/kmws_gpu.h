/*
 * kmws_gpu.h -- C ABI of the MI355X (gfx950) WebSocket frame codec.
 *
 * Drop-in boundary for kuma's RFC 6455 codec (reference: src/ws/WSHandler.h:32-91,
 * used by WebSocket::Impl, src/ws/WebSocketImpl.cpp).  Plain C: fixed-width
 * integers, raw pointers and sizes; a HIP stream is passed as `void*`
 * (a hipStream_t, NULL = the default stream).  Every function returns a
 * kmws_status (0 = OK, negative = kuma KMError value, include/kmdefs.h:61-86)
 * unless noted; codec results use kuma's WSError numbering (wsdefs.h:56-67).
 *
 * Three families:
 *  - host codec entries (kmws_encode_header, kmws_decoder_*): the per-connection,
 *    byte-stream state machine that kuma runs on its event-loop thread.  The
 *    decoder parses headers on the host; payload unmasking is done by the GPU
 *    kernels below (batched per feed call).  See DESIGN.md "Boundary".
 *  - loop-level host batches: kmws_rx_batch_* (receive: one GPU batch per
 *    event-loop iteration across reads and connections), kmws_tx_batch_*
 *    (send: one GPU mask launch for every send of an iteration),
 *    kmws_mask_host_chain and kmws_pipeline_* (host-resident frame batches);
 *    synchronous, pinned staging or zero-copy on caller-pinned memory.
 *  - device batch entries (kmws_*_batch, kmws_unpack_headers,
 *    kmws_gather_unmask): stream-ordered, no host sync, no allocation; all
 *    pointers are device pointers; workspace is caller-owned.  The one set-up
 *    call, kmws_unmask_autotune, synchronizes.
 *
 * Bench / test support (arenas, synthetic batches, the device checker) lives
 * in include/kmws_bench.h, outside this boundary.
 */
#ifndef KMWS_GPU_H
#define KMWS_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: kuma KMError values (include/kmdefs.h:61-86) ---- */
typedef int kmws_status;
#define KMWS_OK                    0
#define KMWS_ERR_FAILED           (-1)   /* KMError::FAILED (HIP runtime error) */
#define KMWS_ERR_TIMEOUT          (-6)   /* KMError::TIMEOUT: a host job the device neither finished nor
                                            gave up in time; the device may still write its buffer */
#define KMWS_ERR_INVALID_STATE    (-7)   /* KMError::INVALID_STATE */
#define KMWS_ERR_INVALID_PARAM    (-8)   /* KMError::INVALID_PARAM */
#define KMWS_ERR_BUFFER_TOO_SMALL (-17)  /* KMError::BUFFER_TOO_SMALL */
#define KMWS_ERR_BUFFER_TOO_LONG  (-18)  /* KMError::BUFFER_TOO_LONG (a send of more than 128 segments) */
#define KMWS_ERR_NOT_SUPPORTED    (-19)  /* KMError::NOT_SUPPORTED (no gfx950 device) */

/* The resident worker's job limits (kmws_resident.hip): the masked payloads of
 * one call or one submitted generation, at most KMWS_RESIDENT_MAX_PAYLOADS of
 * them and KMWS_RESIDENT_MAX_BYTES bytes, run on the calling thread's slot of
 * the device's resident grid without a kernel launch; larger jobs, and a job
 * posted while the thread's previous one still runs, launch instead.  The
 * loop helpers (include/kmws_wshandler.hpp) size their generations to fit. */
#define KMWS_RESIDENT_MAX_PAYLOADS 128
#define KMWS_RESIDENT_MAX_BYTES (256u << 10)
/* The byte limit of a CHECKED job: a call or generation that holds a frame
 * checked under kmws_decoder_set_utf8_check runs on the grid up to this many
 * payload bytes and launches above it (the grid validates with one workgroup
 * per 16 KiB part; above 64 KiB a launch's many small blocks are faster).  The
 * payload limit is KMWS_RESIDENT_MAX_PAYLOADS as for every job.  The loop
 * helpers size generations by KMWS_RESIDENT_MAX_BYTES whatever the check: with
 * it on, a generation between the two limits launches. */
#define KMWS_RESIDENT_MAX_CHECKED_BYTES (64u << 10)

/* ---- device selection (SURVEY 8 e): which GPU a loop thread's objects use ----
 * kuma runs a pool of event-loop threads (test/client/main.cpp:20,
 * test/server/main.cpp:22) and every connection's bytes arrive on its loop
 * thread (TcpConnection.cpp:229).  Every `device` argument below also accepts
 * KMWS_DEVICE_AUTO: the calling thread's device, kmws_thread_device() -- the
 * one kmws_set_thread_device pinned, else chosen once for the thread by the
 * process's policy: NUMA (default: round robin over the GPUs on the NUMA node
 * of the CPU the thread runs on, over all GPUs when that node has none),
 * ROUND_ROBIN (over all GPUs, in the order threads first ask), FIRST (device
 * 0).  So each loop thread's payloads cross its own GPU's PCIe link into its
 * own pinned staging; host DRAM is what the threads still share.  A thread's
 * device does not change once chosen.  The library reads no environment. */
#define KMWS_DEVICE_AUTO (-1)
enum kmws_device_policy { KMWS_DEVICE_POLICY_NUMA = 0, KMWS_DEVICE_POLICY_ROUND_ROBIN = 1,
                          KMWS_DEVICE_POLICY_FIRST = 2 };
kmws_status kmws_set_device_policy(int policy);  /* process-wide; threads that chose keep their device */
/* Pins the calling thread to `device` (KMWS_DEVICE_AUTO: back to the policy for
 * objects created later).  KMWS_ERR_NOT_SUPPORTED: no such gfx950 device. */
kmws_status kmws_set_thread_device(int device);
/* The calling thread's device (>= 0), or KMWS_ERR_NOT_SUPPORTED without a
 * gfx950 device. */
int         kmws_thread_device(void);
/* Claims the calling thread's slot of `device`'s resident grid now (the
 * synchronous entries and batch submits otherwise claim it at their first
 * job) and registers the thread-exit hook that gives it back -- after every
 * thread_local object constructed before this call returned, i.e. after a
 * thread_local loop object whose constructor calls it (kmws::RxLoop, TxLoop),
 * so that object's destructor still flushes on the slot.  A job asked for
 * after the hook ran launches instead.  Returns the slot, or negative: no
 * slot free (jobs launch), the worker is off for this thread, or no device. */
int         kmws_thread_attach(int device);

/* ---- codec results: WSError (src/ws/wsdefs.h:56-67) ---- */
enum kmws_ws_error {
    KMWS_WS_NOERR = 0, KMWS_WS_NEED_MORE_DATA = 1, KMWS_WS_HANDSHAKE = 2,
    KMWS_WS_INVALID_PARAM = 3, KMWS_WS_INVALID_STATE = 4, KMWS_WS_INVALID_FRAME = 5,
    KMWS_WS_INVALID_LENGTH = 6, KMWS_WS_PROTOCOL_ERROR = 7, KMWS_WS_CLOSED = 8,
    KMWS_WS_DESTROYED = 9
};

/* WSMode (wsdefs.h:69-72) */
enum kmws_mode { KMWS_MODE_CLIENT = 0, KMWS_MODE_SERVER = 1 };

/* WSOpcode (wsdefs.h:47-54) */
enum kmws_opcode { KMWS_OP_CONTINUE = 0, KMWS_OP_TEXT = 1, KMWS_OP_BINARY = 2,
                   KMWS_OP_CLOSE = 8, KMWS_OP_PING = 9, KMWS_OP_PONG = 10 };

#define KMWS_MASK_KEY_SIZE   4          /* WS_MASK_KEY_SIZE, wsdefs.h:36 */
#define KMWS_MAX_HEADER_SIZE 14         /* WS_MAX_HEADER_SIZE, wsdefs.h:37 */
#define KMWS_MAX_FRAME_DATA_LENGTH (10u * 1024u * 1024u)  /* WSHandler.cpp:110 */

/* FrameHeader (wsdefs.h:74-88) with the bitfields widened to bytes.  `reserved`
 * is 0, except during the frame callback of a decoder with the UTF-8 check on
 * (kmws_decoder_set_utf8_check): then it holds the frame's KMWS_UTF8_* value. */
typedef struct kmws_frame_hdr {
    uint8_t  fin, rsv1, rsv2, rsv3, opcode, mask, plen, reserved;
    uint64_t xpl64;                      /* union xpl: xpl16 = low 16 bits */
    uint8_t  maskey[KMWS_MASK_KEY_SIZE]; /* wire order */
    uint32_t length;
} kmws_frame_hdr;

/* Frame descriptor in HBM (16 B): payload at base+off, len bytes, key = the
 * 4 wire key bytes read as a little-endian u32 (== *(uint32_t*)hdr.maskey,
 * WebSocketImpl.cpp:386). */
typedef struct kmws_desc {
    uint64_t off;
    uint32_t len;
    uint32_t key;
} kmws_desc;

/* Per-frame flags for the pack kernels: bits 0-7 = header byte 0
 * (fin<<7 | rsv1<<6 | rsv2<<5 | rsv3<<4 | opcode), bit 8 = mask. */
#define KMWS_FLAG_MASK 0x100u
static inline uint16_t kmws_make_flags(int fin, int rsv1, int rsv2, int rsv3, int opcode, int mask)
{
    return (uint16_t)((fin ? 0x80 : 0) | (rsv1 ? 0x40 : 0) | (rsv2 ? 0x20 : 0) |
                      (rsv3 ? 0x10 : 0) | (opcode & 0x0F) | (mask ? KMWS_FLAG_MASK : 0));
}

/* ======================= host codec entries ======================= */

/* WSHandler::encodeFrameHeader (WSHandler.cpp:46-106).  Returns the header
 * length (2, 4 or 10, +4 when masked); out must hold 14 bytes. */
int kmws_encode_header(const kmws_frame_hdr* hdr, uint8_t out[KMWS_MAX_HEADER_SIZE]);

/* Length of the header kmws_encode_header would write (2/4/10 + 4*mask). */
int kmws_header_size(uint32_t length, int mask);

/* ---- streaming decoder: WSHandler (WSHandler.h:32-91) ---- */
typedef struct kmws_decoder kmws_decoder;

/* Frame callback: WSHandler::FrameCallback (WSHandler.h:35).  The payload
 * view is valid only during the call (WSHandler.cpp:285).  Return nonzero if
 * the callback destroyed the owner; the decoder then returns
 * KMWS_WS_DESTROYED without touching itself (DESTROY_DETECTOR, :284-287). */
typedef int (*kmws_frame_cb)(const kmws_frame_hdr* hdr, uint8_t* payload, size_t len, void* user);

/* mode: kmws_mode.  device: HIP device used for payload unmasking. */
kmws_decoder* kmws_decoder_create(int mode, int device);
void          kmws_decoder_destroy(kmws_decoder* dec);
void          kmws_decoder_set_mode(kmws_decoder* dec, int mode);   /* WSHandler::setMode */
void          kmws_decoder_reset(kmws_decoder* dec);                /* WSHandler::reset, :324-327 */

/* WSHandler::handleData (WSHandler.cpp:41-44 -> decodeFrame :108-280).
 * Same return values and callback sequence; masked payloads are unmasked by
 * the GPU (one batched launch per call) and, as in kuma, in place in `data`
 * when a frame lies wholly inside it.  If `data` is pinned host memory the
 * kernel unmasks it there directly (zero-copy, rewriting the 16-B hulls of
 * those payloads); otherwise payloads go through a pinned staging copy.
 * Returns a kmws_ws_error value, or a negative kmws_status if the GPU step
 * failed. */
int kmws_decoder_feed(kmws_decoder* dec, uint8_t* data, size_t len, kmws_frame_cb cb, void* user);

/* In-place contract of kmws_decoder_feed for a PAGEABLE chunk (on by default).
 * Off: a masked payload lying in the chunk is delivered as a view of its
 * unmasked pinned staging copy and the chunk keeps its masked bytes -- one
 * host copy fewer per read.  kuma cannot tell the difference: its read buffer
 * is not touched after handleData returns (TcpConnection.cpp:229-238) and the
 * frame callback only sees the view (WSHandler.cpp:285).  Pinned chunks are
 * always unmasked in place (zero-copy). */
void kmws_decoder_set_in_place(kmws_decoder* dec, int on);

/* Opt-in UTF-8 check of text messages on the host path (RFC 6455 5.6 / 8.1),
 * off by default; NULL is a no-op.  With it on, kmws_decoder_feed and
 * kmws_decoder_feed_deferred / kmws_rx_batch_* (so RxLoop too) deliver every
 * frame with a KMWS_UTF8_* value (defined below, with their exact meaning, at
 * kmws_utf8_validate) in kmws_frame_hdr.reserved while its callback runs --
 * kmws_frame_utf8(hdr) reads it.  With the check off the byte is 0
 * (== KMWS_UTF8_NOT_TEXT), as it always was.  Per connection the values are
 * exactly kmws_utf8_validate's for one stream, the stream being everything this
 * decoder was fed since it was created or kmws_decoder_reset: OK / BAD /
 * AFTER_BAD / NOT_TEXT as defined there, including rule (b) -- a FIN that ends
 * inside a code point, which an empty frame can do.  The message state lives in
 * the decoder, survives across feeds and across rx generations in flight, and
 * is cleared by kmws_decoder_reset.  The verdict is advisory: every frame is
 * unmasked and delivered as without the check and the feeds' return values do
 * not change; the application closes with 1007 when it sees KMWS_UTF8_BAD.
 * Switch only between messages and while none of the decoder's frames are
 * pending in a batch.
 *
 * How: the host parser, which walks each connection's frames in order anyway,
 * keeps the message state (a few instructions per frame); the payload bytes
 * are checked by the GPU in the pass that unmasks them.  Unmasked frames of a
 * CLIENT-mode decoder, which otherwise need no GPU work, are sent through that
 * pass for the check alone (nothing is stored to them); empty frames never need
 * the GPU.  Routing: a call or generation that holds a checked frame (a text
 * message's frame with payload) is posted to the calling thread's slot of the
 * resident worker like any other -- the grid validates in the pass that
 * unmasks, so text traffic in reads of up to 64 KiB keeps the launch-free
 * path.  It is launched when it has more than KMWS_RESIDENT_MAX_PAYLOADS
 * payloads or more than KMWS_RESIDENT_MAX_CHECKED_BYTES (64 KiB) payload bytes
 * -- a lower byte limit than the KMWS_RESIDENT_MAX_BYTES of a job without a
 * checked frame -- and, like every job, when the thread's slot is still busy
 * with its previous job or there is no slot (all taken, or the worker switched
 * off).  A synchronous feed of one <= 64 KiB read always fits; an RxBatch /
 * RxLoop generation, which the helpers let grow to 128 KiB and more, launches
 * once it passes 64 KiB with the check on: flush or submit earlier to stay on
 * the grid.  The first
 * checked job of a process on a device also launches if it meets a running
 * grid: that grid is the kernel without the check and is asked to leave; every
 * grid after it validates.  Verdicts, bytes and return values are the same
 * whichever way a job goes.  Binary and control-only generations, and
 * everything with the check off, go exactly as before.  If
 * the GPU step of a call or generation fails, its frames are dropped as
 * without the check, and the message that was open across them is no longer
 * checkable: its later frames report KMWS_UTF8_NOT_TEXT until the next message
 * head.  Not done: the reason text of a CLOSE frame (kmws_decoder_set_proto_check
 * below judges it: KMWS_PROTO_CLOSE_REASON) and the byte offset of the error. */
void kmws_decoder_set_utf8_check(kmws_decoder* dec, int on);
/* The KMWS_UTF8_* value of a frame, valid during its frame callback.  Also
 * exported as a function for callers that cannot use a macro. */
uint8_t kmws_frame_utf8(const kmws_frame_hdr* hdr);
#define kmws_frame_utf8(h) ((h)->reserved)

/* Opt-in check of the frame sequence and the CLOSE body on the host path (RFC
 * 6455 5.2, 5.4, 5.5, 7.4), off by default; NULL is a no-op.  With it on,
 * kmws_decoder_feed and kmws_decoder_feed_deferred / kmws_rx_batch_flush /
 * kmws_rx_batch_poll (so RxLoop too) judge every frame by the rules of
 * kmws_proto_check (below, with the KMWS_PROTO_* values) for one stream, the
 * stream being everything this decoder was fed since it was created or
 * kmws_decoder_reset, which returns the state to IDLE.  rsv_allowed: the RSV
 * bits (0x40, 0x20, 0x10) a data message's head may carry; other bits of it
 * are ignored.  kmws_decoder_frame_proto reads the verdict of the frame whose
 * callback is running on dec; outside a callback, with the check off, or for
 * NULL it is 0 (== KMWS_PROTO_OK).  The verdict is advisory: bytes, callbacks
 * and return values do not change; the application closes with 1002, or with
 * 1007 for KMWS_PROTO_CLOSE_REASON.
 *
 * How: the parser computes the verdict when it completes a frame -- the state
 * is one byte and a CLOSE payload is at most 125 contiguous bytes by then,
 * unmasked into a private copy for the check -- so this check needs no GPU.
 * The verdict waits with the queued frame, beside its UTF-8 view, and is
 * published on the decoder just before the frame's callback and cleared after
 * it.  A frame that is parsed but never delivered (its GPU step failed, or
 * kmws_rx_batch_discard) still counts for the state.  On this path
 * KMWS_PROTO_HEADER, KMWS_PROTO_CONTROL and KMWS_PROTO_AFTER_CLOSE cannot
 * occur: the decoder stops at a header error, at a control frame without FIN
 * or above 125 bytes, and after a CLOSE, as kuma does. */
void kmws_decoder_set_proto_check(kmws_decoder* dec, int on, uint32_t rsv_allowed);
int  kmws_decoder_frame_proto(const kmws_decoder* dec);

/* WSHandler::handleDataMask(key, KMBuffer&) (WSHandler.cpp:312-322) and, with
 * nseg == 1, handleDataMask(key, data, len) (:303-310) for HOST buffers: the
 * segments of a chain are masked in place with the key phase continuing
 * across segments.  Runs on the GPU (gathered into pinned staging, one
 * unmask launch, scattered back); synchronous; per-thread staging. */
kmws_status kmws_mask_host_chain(const uint8_t key[KMWS_MASK_KEY_SIZE], uint8_t* const* segs, const size_t* lens,
                                 size_t nseg, int device);

/* ---- deferred delivery: one GPU batch per event-loop iteration (SURVEY f-1) ----
 * kuma calls handleData once per 64 KiB socket read per connection; a GPU
 * round trip per call costs more than the scalar unmask it replaces.  A loop
 * thread instead feeds every read of every connection with
 * kmws_decoder_feed_deferred (headers parsed and validated immediately, same
 * return values as kmws_decoder_feed; payloads copied into the batch) and
 * once per iteration either calls kmws_rx_batch_flush -- one GPU unmask over
 * all staged payloads, then every deferred callback in feed order -- or,
 * asynchronously, kmws_rx_batch_submit (enqueues the unmask of the iteration's
 * frames and returns at once) and kmws_rx_batch_poll at the next iterations
 * (delivers the callbacks of every submitted generation whose unmask has
 * finished, in submit order; wait != 0: all of them), so the GPU round trip
 * overlaps the loop's socket reads (the EventLoop::post pattern,
 * kmapi.h:204-210).  Payload views point into the batch (or the attached
 * ring) and are valid during the callback; the caller's chunk is not
 * modified.  A callback returning nonzero ("destroyed") drops every other frame
 * of that decoder still held by the batch: the rest of the generation, later
 * generations in flight and the generation being fed.  Destroy a decoder only after its
 * frames were delivered or after kmws_rx_batch_discard (which also covers
 * submitted generations).  Do not mix kmws_decoder_feed and deferred feeds on
 * one decoder while its frames are pending. */
typedef struct kmws_rx_batch kmws_rx_batch;
kmws_rx_batch* kmws_rx_batch_create(int device);      /* NULL without a gfx950 device */
void           kmws_rx_batch_destroy(kmws_rx_batch* b);
int            kmws_decoder_feed_deferred(kmws_decoder* dec, kmws_rx_batch* b, const uint8_t* data, size_t len,
                                          kmws_frame_cb cb, void* user);
int            kmws_rx_batch_flush(kmws_rx_batch* b);  /* frames delivered, or negative status */
int            kmws_rx_batch_submit(kmws_rx_batch* b); /* frames submitted (0: none), or negative status */
int            kmws_rx_batch_poll(kmws_rx_batch* b, int wait);  /* frames delivered, or negative status */
int            kmws_rx_batch_pending(const kmws_rx_batch* b);   /* frames fed, not yet submitted */
uint64_t       kmws_rx_batch_pending_bytes(const kmws_rx_batch* b);  /* their masked payload bytes */
int            kmws_rx_batch_inflight(const kmws_rx_batch* b);  /* generations submitted, not yet delivered */
/* Optional pinned receive ring (hipHostMalloc / hipHostRegister, e.g.
 * kmws_host_alloc) that the loop reads sockets into: chunks fed from inside it
 * are not copied -- their masked payloads are unmasked in place there
 * (zero-copy), and the callback views point into the ring.  The ring bytes of a
 * frame must stay unmodified until the frame is delivered.  Only while the
 * batch holds no frames; NULL detaches. */
kmws_status    kmws_rx_batch_attach_ring(kmws_rx_batch* b, uint8_t* ring, size_t bytes);
void           kmws_rx_batch_discard(kmws_rx_batch* b, const kmws_decoder* dec);

/* ---- batched send path: one GPU batch per event-loop iteration (SURVEY f-2) ----
 * WebSocket::Impl::sendWsFrame (WebSocketImpl.cpp:381-436) masks the caller's
 * payload in place and packs the header, once per send.  A loop thread
 * instead queues every send of the iteration with kmws_tx_batch_add -- the
 * header is packed at once into hdr_out (length = (uint32_t) payload bytes,
 * :390/:415, then encodeFrameHeader) and the payload segments are queued for
 * masking with hdr->maskey when hdr->mask is set and the payload is not empty
 * (kuma's client mode: mask = 1 and a fresh key per frame, :386/:411; keys are
 * inputs here) -- and masks every queued payload in place with one GPU launch,
 * key phase continuing across a frame's segments: kmws_tx_batch_flush
 * (synchronous), or kmws_tx_batch_submit (returns a ticket at once) and
 * kmws_tx_batch_poll(ticket) (1 once every generation up to the ticket is
 * masked and back in the caller's buffers, 0 while in flight; wait != 0
 * blocks), so the loop fills and submits the next iteration's sends while
 * this one's masks run.  The segments must stay valid and unmodified until
 * their generation completed; the iovec list for the socket is then [hdr_out,
 * segments...] as in :419-431.  A send with more than 128 non-empty segments
 * returns KMWS_ERR_BUFFER_TOO_LONG, and -- as in kuma, which masks before
 * counting iovecs -- its payload is still masked.  Payloads over 4 GiB - 1
 * are refused (KMWS_ERR_INVALID_PARAM). */
typedef struct kmws_tx_batch kmws_tx_batch;
kmws_tx_batch* kmws_tx_batch_create(int device);      /* NULL without a gfx950 device */
void           kmws_tx_batch_destroy(kmws_tx_batch* b);
/* Returns the header length (2..14) or a negative kmws_status. */
int            kmws_tx_batch_add(kmws_tx_batch* b, const kmws_frame_hdr* hdr, uint8_t* const* segs,
                                 const size_t* lens, size_t nseg, uint8_t hdr_out[KMWS_MAX_HEADER_SIZE]);
/* Masks every queued payload (one launch, synchronous); returns the number of
 * frames masked, or a negative kmws_status.  The batch is empty afterwards. */
int64_t        kmws_tx_batch_flush(kmws_tx_batch* b);
/* Enqueues the mask of every queued payload; returns its ticket (> 0), 0 if
 * nothing was queued, or a negative kmws_status. */
int64_t        kmws_tx_batch_submit(kmws_tx_batch* b);
int            kmws_tx_batch_poll(kmws_tx_batch* b, int64_t ticket, int wait);
int            kmws_tx_batch_pending(const kmws_tx_batch* b);
/* Optional pinned send ring (hipHostMalloc / hipHostRegister) the loop builds
 * its outgoing payloads in: segments inside it are masked in place there
 * (zero-copy, one launch), the others go through pinned staging.  Only while
 * no sends are queued or in flight (KMWS_ERR_INVALID_STATE otherwise); NULL
 * detaches. */
kmws_status    kmws_tx_batch_attach_ring(kmws_tx_batch* b, uint8_t* ring, size_t ring_bytes);

/* ======================= device batch entries ======================= */

/* Number of HIP devices of arch gfx950 visible (0 => device entries return
 * KMWS_ERR_NOT_SUPPORTED).  Never falls back to the CPU. */
int kmws_device_count(void);

/* Workspace bytes needed by kmws_unmask_batch for `span` bytes of payload
 * address space (status word + an 8-byte record per 16 KiB tile). */
size_t kmws_unmask_workspace_size(uint64_t span);

/* Batched in-place unmask (replaces WSHandler::handleDataMask, WSHandler.cpp:
 * 291-310, for a whole batch).  Frame i's bytes base[off .. off+len) are XORed
 * with key byte (j % 4) for payload position j.  Preconditions: descs sorted
 * by off, non-overlapping, off+len <= span; base 16-byte aligned.  The kernel
 * rewrites whole 16-byte words of each frame's aligned hull (bytes outside a
 * payload keep their value); nothing may write those hull bytes concurrently.
 * A precondition violation sets the workspace status word (kmws_read_status)
 * and leaves the payload untouched. */
kmws_status kmws_unmask_batch(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                              void* workspace, size_t workspace_bytes, void* stream);

/* kmws_unmask_batch in two stream-ordered halves: `plan` validates the
 * descriptors and builds the tile map in the workspace; `apply` runs the
 * unmask kernel with the default schedule.  A plan stays valid for the same
 * (descs, n, span). */
kmws_status kmws_unmask_plan(uint64_t span, const kmws_desc* descs, uint32_t n, void* workspace,
                             size_t workspace_bytes, void* stream);
kmws_status kmws_unmask_apply(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                              const void* workspace, size_t workspace_bytes, void* stream);

/* Unmask schedules.  The apply grid is one block per 16 KiB tile; a schedule
 * says which tiles the resident blocks stream at once and how the payload is
 * stored.  Placement kind (low byte): */
#define KMWS_SCHED_GROUPED_RUNS 0   /* XCDs in 2 groups, runs of 16 tiles in each group's half
                                       (the default below a mean frame region of 16 KiB) */
#define KMWS_SCHED_IN_ORDER     1   /* tile = block */
#define KMWS_SCHED_SPLIT2       2   /* blocks dealt over 2 far-apart parts of the span */
#define KMWS_SCHED_SPLIT8       3   /* ... over 8 parts */
#define KMWS_SCHED_XCD_RUNS     4   /* runs of 16 tiles per XCD */
#define KMWS_SCHED_SPLIT4       5   /* ... over 4 parts (the default from a 16 KiB mean region) */
/* Store policy of the payload: streaming by default (neither bit, or
 * KMWS_SCHED_NT_STORES): for batches whose mean frame region is 16 KiB or
 * more, `nt sc1` buffer stores, which do not keep the line in the XCD's L2 --
 * the fastest of nt / nt sc1 / sc1 / sc0 sc1 on the 64 GiB aligned batch and
 * on the packed wire; below that, `nt` stores, which cfg3's Zipf wire needs
 * (profiles/p01_unmask_tilerec_policy_ab.txt).
 * KMWS_SCHED_TEMPORAL_STORES stores plain and keeps the lines in L2
 * (written back on eviction) -- slower on plain allocations of every layout
 * measured, a candidate the autotune times.  At most one bit. */
#define KMWS_SCHED_NT_STORES       (1 << 29)
#define KMWS_SCHED_TEMPORAL_STORES (1 << 30)

/* kmws_unmask_apply with an explicit schedule (schedule < 0: the default,
 * kmws_unmask_default_schedule).  The library keeps no schedule state: a
 * schedule belongs to the caller's plan of one batch (e.g. the code
 * kmws_unmask_autotune returned for it) and is passed on every apply, like the
 * descriptors.  An invalid code returns KMWS_ERR_INVALID_PARAM. */
kmws_status kmws_unmask_apply_sched(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                                    const void* workspace, size_t workspace_bytes, int schedule, void* stream);

/* The schedule kmws_unmask_apply / kmws_unmask_batch use: split 4 from a mean
 * frame region of 16 KiB (span / n), grouped XCD runs below; non-temporal
 * stores. */
int kmws_unmask_default_schedule(uint64_t span, uint32_t n);

/* Optional one-time tuning of ONE batch (like a cuDNN benchmark pass): runs
 * every placement kind with both store policies on this batch, two launches
 * per timing (the XOR applied twice leaves the payload unchanged), in one
 * warm-up round and two timed rounds, a schedule's time being the lower of its
 * two; times them with events on
 * `stream` (synchronizes) and returns the fastest schedule code (or a negative
 * status) for the caller to pass to kmws_unmask_apply_sched.  Nothing is
 * recorded: the next batch, on any workspace, gets the default unless its
 * caller passes a schedule. */
int kmws_unmask_autotune(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Read (synchronously) the status word of a workspace after a batch call, a
 * bit set: 0 = OK, 1 = descriptor precondition violated (or the output would
 * exceed dst_cap), 2 = header error seen, 4 = a scan timed out waiting for a
 * predecessor tile's state (kmws_pack_headers, and kmws_encode_batch /
 * kmws_gather_unmask in their chunk form: never seen with in-order workgroup
 * dispatch).  The offsets those calls write (wire_off, dst_off) are valid
 * only when the status is 0; with bit 1 or 4 set nothing is stored in dst. */
kmws_status kmws_read_status(const void* workspace, uint32_t* status_out, void* stream);

/* ---- batched header pack / unpack (device) ---- */

/* Workspace bytes for kmws_encode_batch / kmws_gather_unmask with n frames
 * and an output capacity of dst_cap bytes.  The copy form follows dst_cap / n
 * (below 16 KiB per frame: 4 KiB output chunks, one wave each, 8 B of
 * workspace per chunk; from it: per-frame edge words and 32 B per 4 KiB
 * output unit), so size the workspace with the dst_cap the call will pass. */
size_t kmws_copy_workspace_size(uint32_t n, uint64_t dst_cap);

/* Batched frame encode: for frame i, WSHandler::encodeFrameHeader
 * (WSHandler.cpp:46-106) of {flags[i], len, key} followed by the payload
 * src[descs[i].off .. +len) masked with key when flags[i] & KMWS_FLAG_MASK
 * (WebSocketImpl.cpp:381-404), all frames back to back in dst.  wire_off
 * (n+1 entries, device) receives each frame's header offset and, in
 * wire_off[n], the total wire size.  If the total exceeds dst_cap nothing is
 * written and the workspace status word is set.  wire_off and dst are valid
 * only when the status (kmws_read_status) is 0 afterwards.  src and dst 16-B
 * aligned; source payloads may overlap or sit anywhere in src. */
kmws_status kmws_encode_batch(const uint8_t* src, const kmws_desc* descs, const uint16_t* flags, uint32_t n,
                              uint8_t* dst, uint64_t dst_cap, uint64_t* wire_off, void* workspace,
                              size_t workspace_bytes, void* stream);

/* Workspace bytes for kmws_pack_headers with n frames. */
size_t kmws_pack_headers_workspace_size(uint32_t n);

/* Batched header pack only -- the device form of kuma's send iovec
 * {header, payload} (WebSocketImpl.cpp:381-404, :419-431): frame i's header,
 * WSHandler::encodeFrameHeader (WSHandler.cpp:46-106) of {flags[i],
 * descs[i].len, descs[i].key}, is written to the 16-byte slot hdr + 16 i (its
 * hdr_len[i] = 2..14 bytes first, the rest of the slot zero).  The payloads are
 * not touched: mask them in place with kmws_unmask_batch (XOR is its own
 * inverse), as sendWsFrame masks the caller's buffer (:388), on descriptors
 * whose key is 0 for every frame whose flags clear KMWS_FLAG_MASK (the header
 * then says unmasked; a nonzero key there would still be applied).  wire_off
 * (n+1 entries, may be NULL) receives the offsets the frames would have back
 * to back on the wire (exclusive scan of header + payload bytes) and the total
 * in wire_off[n]; it needs the workspace (a status word and one 8-byte scan
 * state per 2048 frames, cleared by the call; one pass over the descriptors).
 * wire_off is valid only when the workspace status (kmws_read_status) is 0
 * afterwards.  hdr 16-B aligned. */
kmws_status kmws_pack_headers(const kmws_desc* descs, const uint16_t* flags, uint32_t n, uint8_t* hdr,
                              uint8_t* hdr_len, uint64_t* wire_off, void* workspace, size_t workspace_bytes,
                              void* stream);

/* Workspace bytes for kmws_unpack_headers. */
size_t kmws_unpack_workspace_size(void);

/* Descriptor-indexed header unpack + validation, one frame per hdr_off entry
 * (offsets ascending, each frame ending by the next header): the HDR1..MASKEY
 * rules of WSHandler::decodeFrame (WSHandler.cpp:118-234) for `mode`,
 * including the 127-class length quirk.  Per frame: out_desc = {payload
 * offset in wire, len, key (0 if unmasked)}, out_flags = header byte 0 |
 * mask << 8 (may be NULL), out_err = WSError (may be NULL): 1 truncated,
 * 6 bad length, 7 protocol error, 5 frame overruns the next header -- in the
 * reference's order: a non-FIN control byte is 7 even as the wire's last byte
 * (HDR1, :126-130), every other rule waits for the bytes it reads.  Error
 * frames get len 0.  Any error sets status bit 2. */
kmws_status kmws_unpack_headers(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n,
                                int mode, kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err,
                                void* workspace, size_t workspace_bytes, void* stream);

/* kmws_unpack_headers and kmws_unmask_batch fused: the descriptor-indexed
 * decode in place, as kuma unmasks in the caller's buffer (WSHandler.cpp:
 * 247-260).  One kernel parses every header (the kmws_unpack_headers rules and
 * outputs) and writes the unmask plan -- frame i's region is [hdr_off[i],
 * hdr_off[i+1]) -- then the unmask kernel runs on the wire in place with
 * `schedule` (< 0: the default).  workspace: kmws_unmask_workspace_size(wire_len);
 * wire 16-byte aligned.  A header error sets out_err and status bit 2 and
 * leaves that frame masked (len 0), the others are unmasked; offsets out of
 * order or past wire_len set status bit 1 and nothing is unmasked. */
kmws_status kmws_unpack_unmask(uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                               kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err, void* workspace,
                               size_t workspace_bytes, int schedule, void* stream);

/* Out-of-place unmask: frame i's payload src[descs[i].off .. +len) XOR its key
 * is written densely to dst at dst_off[i] (exclusive scan of len; n+1
 * entries, dst_off[n] = total).  Nothing is written if total > dst_cap.
 * dst_off and dst are valid only when the workspace status is 0 afterwards. */
kmws_status kmws_gather_unmask(const uint8_t* src, const kmws_desc* descs, uint32_t n, uint8_t* dst,
                               uint64_t dst_cap, uint64_t* dst_off, void* workspace, size_t workspace_bytes,
                               void* stream);

/* kmws_unpack_headers and kmws_gather_unmask fused: the header parse runs
 * inside the gather's first (scan) kernel, which writes out_desc / out_flags /
 * out_err exactly as kmws_unpack_headers does; the payloads are then gathered
 * densely into dst as kmws_gather_unmask does (error frames: len 0).
 * workspace: kmws_copy_workspace_size(n, dst_cap); wire and dst 16-byte
 * aligned.  Status bit 2: a header error was seen. */
kmws_status kmws_unpack_gather(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                               kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err, uint8_t* dst,
                               uint64_t dst_cap, uint64_t* dst_off, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Host: walk the header chain of a wire image (WSHandler.cpp:108-280 state
 * order, reading only header bytes and skipping payloads) and record each
 * header offset.  Stops after `cap` frames, after a frame that is truncated
 * or has an invalid length -- a 126-class length below 126, a 127-class length
 * with bit 63 set or above KMWS_MAX_FRAME_DATA_LENGTH, where the reference
 * returns INVALID_LENGTH (:166-170, :183-193) -- (recorded, so
 * kmws_unpack_headers reports it), or after a CLOSE frame (the reference stops
 * parsing there, :265-268).  The walk has no mode and does not stop at a
 * protocol error (kmws_unpack_headers reports those per frame).
 * *consumed = bytes covered by the recorded complete frames. */
kmws_status kmws_find_headers(const uint8_t* wire, uint64_t len, uint64_t* hdr_off, uint32_t cap,
                              uint32_t* n_out, uint64_t* consumed);

/* Device: the same header-chain walk as kmws_find_headers, one lane per
 * stream, for many streams at once (boundary discovery is serial within a
 * stream -- frame k+1 starts where frame k's header says -- so a batch gets its
 * parallelism from connections; SURVEY 8 "hard parts").  Stream s is
 * wire[stream_off[s] .. stream_off[s+1]) (stream_off: n_streams+1 ascending
 * entries, stream_off[n_streams] <= wire_len; a stream reaching past wire_len
 * is cut there).  Its header offsets (absolute,
 * into wire) go to hdr_off[s * cap .. s * cap + n_out[s]); consumed[s] (may be
 * NULL) = bytes of stream s covered by its complete frames.  Stopping rules as
 * kmws_find_headers: cap frames, a truncated frame or invalid length (recorded),
 * or after a CLOSE frame.  All pointers device memory.
 * A stream's last recorded frame was recorded without being consumed -- cut by
 * the stream's end, or refused for its length: the outputs do not say which --
 * iff its offset equals stream_off[s] + consumed[s].  Leave that one out of the
 * flat hdr_off list the kmws_unpack_* entries take: they bound a frame's header
 * bytes by wire_len only, so a cut header in front of another stream's bytes
 * would be completed with them.  Parse it alone instead (kmws_unpack_headers,
 * n = 1, wire_len = the stream's end): out_err 1 means wait for the next read,
 * anything else fails the connection ("The receive
 * loop of a device batch"; tests/test_gpu_server_loop.py). */
kmws_status kmws_find_headers_streams(const uint8_t* wire, uint64_t wire_len, const uint64_t* stream_off,
                                      uint32_t n_streams, uint64_t* hdr_off, uint32_t cap, uint32_t* n_out,
                                      uint64_t* consumed, void* stream);

/* ---- UTF-8 validation of text messages (opt-in; RFC 6455 5.6 / 8.1) ----
 * kuma hands text payloads to the application as they are (onWsFrame,
 * WebSocketImpl.cpp:268-301); a server that wants the check the RFC asks for
 * (fail the connection with 1007) calls this on the device batch instead of
 * walking every unmasked payload on the host.  Nothing else changes behaviour.
 *
 * Per-frame result: */
#define KMWS_UTF8_NOT_TEXT  0  /* not checked: control frame, frame of a binary or RSV1 message,
                                  CONTINUE with no open message */
#define KMWS_UTF8_OK        1  /* checked; the message's bytes through this frame are a prefix of a
                                  well-formed UTF-8 string, and a whole one if this frame has FIN */
#define KMWS_UTF8_BAD       2  /* the first frame of its message at which that stops holding */
#define KMWS_UTF8_AFTER_BAD 3  /* a later frame of a message already reported BAD (this batch or,
                                  through the carry, an earlier one) */

/* State of one stream between two batches: 8 bytes, all zero = between messages, otherwise
 * opaque; pass back what the previous call wrote for that stream. */
typedef struct kmws_utf8_carry { uint8_t b[8]; } kmws_utf8_carry;

/* Workspace bytes for kmws_utf8_validate: kmws_unmask_workspace_size(span) plus
 * about 12 B per frame and 8 B per stream. */
size_t kmws_utf8_workspace_size(uint64_t span, uint32_t n, uint32_t n_streams);

/* Stream-ordered, no host sync, no allocation, kernel nodes only (capturable).
 * descs / base / span: kmws_unmask_batch's preconditions (sorted, non-
 * overlapping, in span; base 16-byte aligned); a violation sets status bit 1
 * and out / carry_out are then not valid.  The payload is never written.
 * flags[i]: header byte 0 | mask << 8, what kmws_unpack_headers writes to
 * out_flags.  payload_masked != 0: the bytes in memory are still masked with
 * descs[i].key (as before an unmask; the key is applied in registers);
 * == 0: they are plain and key is ignored -- so the call runs before or after
 * kmws_unmask_batch / kmws_unpack_unmask, or on kmws_gather_unmask's dense
 * output with descriptors built from dst_off.
 * stream_first: n_streams + 1 ascending frame indices, [0] == 0, [n_streams]
 * == n; stream s is frames [stream_first[s], stream_first[s+1]) in wire order
 * and may be empty; NULL with n_streams == 1: the batch is one stream.  A
 * malformed array sets status bit 1.  carry_in (may be NULL: every stream
 * starts between messages) and carry_out (may be NULL) hold one entry per
 * stream; an empty stream's carry_out equals its carry_in.  n == 0: KMWS_OK,
 * carry_out = carry_in.  out: n bytes.
 *
 * Per stream, in frame order: a control frame (opcode >= 8) gets 0 and does
 * not touch the message state; opcode 1-7 starts a message, replacing any
 * unfinished one (whether that is a protocol error is the parser's business),
 * which is checked iff opcode == 1 and RSV1 == 0 (a compressed message's bytes
 * are deflate data); opcode 0 belongs to the open message (none: 0); FIN on a
 * non-control frame closes the message.  Well-formed: RFC 3629 section 4 /
 * Unicode table 3-7.  A frame is BAD iff it is the first of its message at
 * which (a) the message's bytes through that frame are not a prefix of any
 * well-formed string, or (b) it has FIN and they end inside a code point --
 * which an empty FIN frame can do.
 *
 * Not done here: the reason text of a CLOSE frame (kmws_proto_check below
 * judges it: KMWS_PROTO_CLOSE_REASON); the byte offset of the error.  Every payload pass has the check
 * fused in: the in-place unmask, the gather and the reframe
 * (kmws_unmask_utf8_batch, kmws_gather_unmask_utf8 and kmws_reframe_utf8_batch
 * below), and the host path through
 * kmws_decoder_set_utf8_check -- launched jobs and the resident grid's alike. */
kmws_status kmws_utf8_validate(const uint8_t* base, uint64_t span, const kmws_desc* descs,
                               const uint16_t* flags, uint32_t n, int payload_masked,
                               const uint32_t* stream_first, uint32_t n_streams,
                               const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                               uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- frame-sequence and CLOSE rules per stream (opt-in; RFC 6455 5.2, 5.4, 5.5, 7.4) ----
 * kuma's WSHandler accepts sequences the RFC forbids -- a CONTINUE with no open
 * message (the TODO at WSHandler.cpp:131), a new data head inside a message,
 * reserved opcodes, RSV bits nobody negotiated, any CLOSE body -- and so does
 * this codec, byte for byte.  A server that wants to answer 1002 (and 1007 for a
 * CLOSE reason) without walking every stream's frames on the CPU calls this on
 * the descriptors of a device batch.  Nothing else changes behaviour.
 *
 * Per-frame result.  A stream is IDLE, OPEN (a data message is unfinished),
 * CLOSED or FAILED; every value but OK, and AFTER_*, moves it to FAILED: */
#define KMWS_PROTO_OK             0
#define KMWS_PROTO_RSV            1  /* an RSV bit outside rsv_allowed on a data head (opcode 1, 2), or any
                                        on a CONTINUE or control frame */
#define KMWS_PROTO_OPCODE         2  /* opcode 3-7 or 11-15 */
#define KMWS_PROTO_CONTROL        3  /* a control frame without FIN or longer than 125 bytes */
#define KMWS_PROTO_CONTINUATION   4  /* CONTINUE with no open message */
#define KMWS_PROTO_INTERLEAVED    5  /* opcode 1 or 2 while a message is open */
#define KMWS_PROTO_CLOSE_PAYLOAD  6  /* CLOSE with one payload byte, or a status code outside
                                        1000-1003, 1007-1014, 3000-4999 */
#define KMWS_PROTO_CLOSE_REASON   7  /* CLOSE whose reason (bytes 2..) is not a complete well-formed UTF-8
                                        string: answer 1007 */
#define KMWS_PROTO_AFTER_CLOSE    8  /* any frame after a valid CLOSE */
#define KMWS_PROTO_HEADER         9  /* err[i] != 0: the parser rejected the header */
#define KMWS_PROTO_AFTER_FAIL     10 /* any frame after one of the above (this batch or, through the carry,
                                        an earlier one) */

/* State of one stream between two batches: all zero = IDLE; b[0] = the state
 * (0 IDLE, 1 OPEN, 2 CLOSED, 3 FAILED), b[1..7] = 0. */
typedef struct kmws_proto_carry { uint8_t b[8]; } kmws_proto_carry;

/* Workspace bytes for kmws_proto_check: about 2 B per frame and 3 B per 1024
 * frames or streams. */
size_t kmws_proto_workspace_size(uint32_t n, uint32_t n_streams);

/* Stream-ordered, no host sync, no allocation, three kernel nodes (capturable);
 * the status word is cleared by a kernel.  The first rule that matches decides
 * a frame's own class: err[i] != 0 -> HEADER; a forbidden RSV bit -> RSV; a
 * reserved opcode -> OPCODE; a control frame without FIN or above 125 bytes ->
 * CONTROL; a CLOSE body -> CLOSE_PAYLOAD / CLOSE_REASON.  Then, per stream in
 * frame order: FAILED -> AFTER_FAIL; CLOSED -> AFTER_CLOSE; a nonzero class ->
 * that class, FAILED; CONTINUE when IDLE -> CONTINUATION, FAILED; opcode 1 / 2
 * when OPEN -> INTERLEAVED, FAILED; else OK, after which a CLOSE leaves CLOSED,
 * PING / PONG change nothing and a data frame leaves IDLE with FIN, else OPEN.
 *
 * flags[i]: header byte 0 | mask << 8 (kmws_unpack_headers' out_flags); err
 * (may be NULL: no frame has a header error): its out_err; descs[i].len: the
 * payload length.  rsv_allowed: the RSV bits (0x40, 0x20, 0x10) allowed on a
 * data message's head, e.g. 0x40 with permessage-deflate.  The descriptors
 * need no order.  Only payloads of CLOSE frames with 2 <= len <= 125 and
 * err == 0 are read, only in [off, off + len); one that reaches past span sets
 * status bit 1 and is not read.  payload_masked, stream_first, n_streams,
 * carry_in, carry_out: as kmws_utf8_validate's (NULL stream_first with
 * n_streams == 1; an empty stream's carry_out equals its carry_in; a malformed
 * array sets status bit 1); a carry_in whose b[0] is not 0..3 sets status bit 1.
 * With status bit 1 set out / carry_out are not valid.  The payload is never
 * written.  n == 0: KMWS_OK, carry_out = carry_in.  out: n bytes.
 *
 * KMWS_ERR_INVALID_PARAM: rsv_allowed & ~0x70, then kmws_utf8_validate's checks
 * in its order (n or n_streams >= 2^31; with frames a NULL base, descs, flags,
 * out or workspace; base not 16-byte aligned; no stream, or several without
 * stream_first).  Then KMWS_ERR_BUFFER_TOO_SMALL below
 * kmws_proto_workspace_size(n, n_streams) with frames, then
 * KMWS_ERR_NOT_SUPPORTED without a gfx950 device: there is no CPU fallback
 * (the host path's check, kmws_decoder_set_proto_check, needs no device).
 *
 * Cost: about 20 B read and 3 B written per frame; the lane that owns a CLOSE
 * frame walks its at most 123 reason bytes serially while the 63 other lanes of
 * its wave wait -- CLOSE frames are at most one per connection. */
kmws_status kmws_proto_check(const uint8_t* base, uint64_t span, const kmws_desc* descs, const uint16_t* flags,
                             const uint8_t* err, uint32_t n, int payload_masked, uint32_t rsv_allowed,
                             const uint32_t* stream_first, uint32_t n_streams, const kmws_proto_carry* carry_in,
                             kmws_proto_carry* carry_out, uint8_t* out, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- the message table of a device batch (opt-in) ----
 * The entries above leave per-frame arrays; an application consumes messages.
 * kuma hands fragments up with their FIN flag (data_cb_(buf, is_text, fin)) and
 * lets the application put the message together; behind a device batch that is
 * a serial host walk over every stream's frames.  This call does it on the
 * device: one record per message, in frame order, with where its payload lies,
 * how long it is and whether it may be delivered.  Nothing else changes
 * behaviour; no payload byte is read or written. */
#define KMWS_MSG_NONE   0xFFFFFFFFu  /* msg_of[i] of a control frame or an orphan CONTINUE */
#define KMWS_MSG_BEGIN  1u  /* the message's head is in this batch */
#define KMWS_MSG_END    2u  /* its FIN frame is in this batch */
#define KMWS_MSG_CONTIG 4u  /* pos[last] + len[last] - pos[first] == bytes: its members' payloads
                               are one run at `off` (always so for a one-frame message) */
typedef struct kmws_msg {            /* 48 B */
    uint64_t off;     /* pos[first] */
    uint64_t bytes;   /* payload bytes of its members in this batch */
    uint64_t prior;   /* its payload bytes in earlier batches (from the carry; 0 with BEGIN) */
    uint32_t stream, first, last, frames;   /* first / last member frame index, member count */
    uint8_t  b0;      /* head byte 0 & 0x7F (RSV1-3, opcode), from the carry when continued */
    uint8_t  bits;    /* KMWS_MSG_* */
    uint8_t  utf8;    /* utf8[last]  (0 when utf8  == NULL) */
    uint8_t  proto;   /* proto[last] (0 when proto == NULL) */
    uint32_t reserved;  /* 0 */
} kmws_msg;
/* State of one stream between two batches: all zero = no message open; b[0] = 0x80 | b0,
 * b[1..7] = 0, b[8..15] = prior + bytes of the open message, little endian. */
typedef struct kmws_msg_carry { uint8_t b[16]; } kmws_msg_carry;

/* Workspace bytes for kmws_msg_index: 2 B per frame (whole blocks of 1024) and
 * 56 B per 1024 frames or 8 B per 1024 streams, whichever blocks are more. */
size_t kmws_msg_workspace_size(uint32_t n, uint32_t n_streams);

/* Stream-ordered, no host sync, no allocation, five kernel nodes (capturable);
 * the status word is stored by a kernel.  kmws_utf8_validate's message rule,
 * per stream in frame order: a control frame (opcode >= 8) is no member and
 * does not touch the state; opcode 1-7 (a head) starts a message, replacing an
 * unfinished one, which keeps its record without END (whether that is an error
 * is kmws_proto_check's business), and is its first member; opcode 0 while a
 * message is open is a member, and starts the record when it is the message's
 * first member in this batch (the message is open through the carry: b0 and
 * prior come from carry_in); opcode 0 while none is open is an orphan: no
 * member, the state unchanged; FIN on a member closes the message.  A frame
 * whose header failed to parse arrives as the kmws_unpack_* entries leave it
 * (len 0, flags as parsed) and is treated by its flags like any other; the
 * caller sees it through the proto verdict (HEADER, then AFTER_FAIL, sticky).
 *
 * flags[i]: header byte 0 | mask << 8 (kmws_unpack_headers' out_flags);
 * descs[i].len: the payload length -- nothing else of a descriptor is used
 * unless pos == NULL.  pos: n entries, frame i's payload position in whatever
 * arena the caller will read -- the dst_off of a gather -- or NULL:
 * descs[i].off.  utf8 / proto: the out arrays of kmws_utf8_validate (or a
 * fused payload pass) and kmws_proto_check, or NULL; both kinds of verdict are
 * sticky within a message or stream, so a record carries its last member's
 * values and no reduction is made.  stream_first, n_streams, carry_in,
 * carry_out: as kmws_proto_check's (NULL stream_first with n_streams == 1; an
 * empty stream's carry_out equals its carry_in, and so does that of a stream
 * without a member in this batch; a malformed array sets status bit 1), with
 * kmws_msg_carry entries, which have byte alignment; a carry_in with b[0] in
 * 1..0x7F or a nonzero b[1..7] sets status bit 1.
 *
 * Records come out in frame order of their first member, and so grouped by
 * stream: msgs[0 .. *msg_count), at most msg_cap (n always suffices); msgs is
 * 8-byte aligned.  stream_msg_first (n_streams + 1 entries, may be NULL): the
 * number of records before each stream, [n_streams] == *msg_count.  msg_of (n
 * entries, may be NULL): each frame's record index, or KMWS_MSG_NONE.  A
 * message without CONTIG has a control frame with payload between its
 * fragments (or positions that are not dense): read its members through
 * msg_of / pos.  More records than msg_cap: status bit 1 is set, *msg_count
 * holds the needed number, and msgs, msg_of and carry_out are not valid; they
 * are not valid either when status bit 1 is set for another reason.  n == 0:
 * KMWS_OK, *msg_count = 0, stream_msg_first all 0, carry_out = carry_in; the
 * workspace is not touched.
 *
 * KMWS_ERR_INVALID_PARAM: n or n_streams >= 2^31; a NULL msg_count or
 * workspace; with frames a NULL descs, flags or msgs; with frames no stream, or
 * several without stream_first.  Then KMWS_ERR_BUFFER_TOO_SMALL below
 * kmws_msg_workspace_size(n, n_streams) with frames, then
 * KMWS_ERR_NOT_SUPPORTED without a gfx950 device: there is no CPU fallback.
 *
 * Not done: a gather that leaves control payloads out so that every message is
 * contiguous (CONTIG reports the case); a message size limit (prior + bytes is
 * what a caller needs for 1009); a host-path assembler (the drop-in keeps
 * kuma's per-frame callbacks).
 *
 * carry_out must not overlap carry_in.
 *
 * Cost: three passes over the frames that read 2, 2 + 4 and 2 + 4 B per frame
 * (flags, and the members' lengths out of their 16-byte descriptors), 2 B per
 * frame stored to and reloaded from the workspace, 4 B per frame stored for
 * msg_of, and per message 48 B stored after about 30 B of gathered reads. */
kmws_status kmws_msg_index(const kmws_desc* descs, const uint16_t* flags, const uint64_t* pos,
                           const uint8_t* utf8, const uint8_t* proto, uint32_t n,
                           const uint32_t* stream_first, uint32_t n_streams,
                           const kmws_msg_carry* carry_in, kmws_msg_carry* carry_out,
                           uint32_t* msg_of, kmws_msg* msgs, uint32_t msg_cap, uint32_t* msg_count,
                           uint32_t* stream_msg_first, void* workspace, size_t workspace_bytes, void* stream);

/* ---- in-place unmask and UTF-8 validation in one pass over the payload ----
 * kmws_unmask_batch followed by kmws_utf8_validate reads every payload byte
 * twice; these entries read it once: the words the unmask stores are validated
 * from the registers that hold them.
 *
 * Workspace bytes: kmws_utf8_workspace_size(span, n, n_streams) plus 4 B per
 * 16 KiB of span (the still-masked dword before each tile, saved ahead of the
 * payload pass so that no look-back is read from bytes another block may
 * already have unmasked). */
size_t kmws_unmask_utf8_workspace_size(uint64_t span, uint32_t n, uint32_t n_streams);

/* The two contracts composed.  Afterwards base holds exactly what
 * kmws_unmask_batch(base, span, descs, n, ..) leaves: every frame unmasked
 * whatever its opcode, key-0 frames and bytes outside payloads untouched, the
 * same 16-byte hull rule; out and carry_out hold exactly what
 * kmws_utf8_validate(.., payload_masked = 1, ..) would have written on the
 * still-masked batch.  The verdict is advisory: a BAD message is unmasked like
 * any other.  schedule: a code of kmws_unmask_apply_sched, < 0 = the default;
 * an invalid code returns KMWS_ERR_INVALID_PARAM.  Stream-ordered, no host
 * sync, no allocation, kernel nodes only (capturable); the status word is
 * cleared by a kernel.  With status bit 1 set (descriptors or stream_first
 * malformed) nothing is stored to the payload and out / carry_out are not
 * valid.  Arguments are checked as kmws_utf8_validate checks them, in its
 * order and with its return values; KMWS_ERR_NOT_SUPPORTED without a gfx950
 * device (no CPU fallback).  n == 0: KMWS_OK, carry_out = carry_in. */
kmws_status kmws_unmask_utf8_batch(uint8_t* base, uint64_t span, const kmws_desc* descs,
                                   const uint16_t* flags, uint32_t n,
                                   const uint32_t* stream_first, uint32_t n_streams,
                                   const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                   uint8_t* out, void* workspace, size_t workspace_bytes,
                                   int schedule, void* stream);

/* kmws_unpack_unmask with the validation in its payload pass.  out_desc,
 * out_flags (required here), out_err, the wire bytes and status bits 1 and 2
 * are exactly as after kmws_unpack_unmask; out_utf8 and carry_out are exactly
 * kmws_utf8_validate applied to the out_desc / out_flags this call writes.  A
 * frame with a header error is what kmws_unpack_unmask makes of it -- len 0,
 * flags as parsed -- and is judged as such an empty frame: look at out_err (or
 * status bit 2) before out_utf8.  workspace:
 * kmws_unmask_utf8_workspace_size(wire_len, n, n_streams). */
kmws_status kmws_unpack_unmask_utf8(uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off,
                                    uint32_t n, int mode, kmws_desc* out_desc, uint16_t* out_flags,
                                    uint8_t* out_err, const uint32_t* stream_first, uint32_t n_streams,
                                    const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                    uint8_t* out_utf8, void* workspace, size_t workspace_bytes,
                                    int schedule, void* stream);

/* ---- gather, unmask and UTF-8 validation in one pass over the payload ----
 * kmws_gather_unmask followed by kmws_utf8_validate on its dense output reads
 * that output back right after writing it; these entries validate the words the
 * gather stores from the registers that hold them.
 *
 * Workspace bytes: kmws_copy_workspace_size(n, dst_cap) (rounded up to 256) plus
 * the validator's per-frame and per-stream arrays (about 12 B per frame, 8 B
 * per stream) -- not its tile plan. */
size_t kmws_gather_utf8_workspace_size(uint32_t n, uint64_t dst_cap, uint32_t n_streams);

/* The two contracts composed.  dst, dst_off and the status word are exactly
 * what kmws_gather_unmask leaves for the same src / descs / n / dst / dst_cap
 * (the cap rule: total > dst_cap sets status bit 1 and stores nothing; bit 4 on
 * a look-back timeout); src is never written, src and dst do not overlap, the
 * descriptors need no order in src.  out_utf8 and carry_out are exactly what
 * kmws_utf8_validate(dst, dst_off[n], D, flags, n, 0, stream_first, n_streams,
 * carry_in, carry_out, ..) writes after the plain gather, with D[i] =
 * {dst_off[i], descs[i].len, 0}.  The verdict is advisory: a BAD message is
 * gathered like any other.  flags / stream_first / carry_in / carry_out:
 * kmws_utf8_validate's; a malformed stream_first sets status bit 1 (nothing is
 * stored then).  With status bit 1 or 4 set out_utf8 / carry_out are not valid.
 * Stream-ordered, no host sync, no allocation, kernel nodes only (capturable);
 * the status word is cleared by a kernel.  KMWS_ERR_INVALID_PARAM for a NULL
 * required pointer (dst_off and workspace always; src, descs, flags, dst,
 * out_utf8 with frames), a misaligned src / dst, n or n_streams >= 2^31, NULL
 * stream_first with n_streams != 1, n_streams == 0 with frames; then
 * KMWS_ERR_BUFFER_TOO_SMALL; then KMWS_ERR_NOT_SUPPORTED without a gfx950
 * device (no CPU fallback).  n == 0: KMWS_OK, dst_off[0] = 0, carry_out =
 * carry_in. */
kmws_status kmws_gather_unmask_utf8(const uint8_t* src, const kmws_desc* descs, const uint16_t* flags, uint32_t n,
                                    uint8_t* dst, uint64_t dst_cap, uint64_t* dst_off,
                                    const uint32_t* stream_first, uint32_t n_streams,
                                    const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                    uint8_t* out_utf8, void* workspace, size_t workspace_bytes, void* stream);

/* kmws_unpack_gather with the validation in its payload pass.  out_desc,
 * out_flags (required here), out_err, dst, dst_off and status bits 1, 2 and 4
 * are exactly as after kmws_unpack_gather; out_utf8 and carry_out are exactly
 * kmws_utf8_validate applied to the dense output and the out_flags this call
 * writes.  A frame with a header error is what kmws_unpack_gather makes of it
 * -- len 0, flags as parsed -- and is judged as such an empty frame: look at
 * out_err (or status bit 2, with which out_utf8 / carry_out stay valid) before
 * out_utf8.  Also KMWS_ERR_INVALID_PARAM for a bad mode. */
kmws_status kmws_unpack_gather_utf8(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n,
                                    int mode, kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err,
                                    uint8_t* dst, uint64_t dst_cap, uint64_t* dst_off,
                                    const uint32_t* stream_first, uint32_t n_streams,
                                    const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                    uint8_t* out_utf8, void* workspace, size_t workspace_bytes, void* stream);

/* ---- unmask and re-encode in one pass over the payload (relay) ----
 * A relay -- a chat room, a pub/sub fan-in, a proxy, an echo -- receives masked
 * client frames and sends the same messages on as server frames, unmasked or
 * masked with fresh keys towards an upstream.  kmws_gather_unmask followed by
 * kmws_encode_batch moves every payload byte four times; both keys are indexed
 * by payload position mod 4, so unmasking with one and masking with the other
 * is one XOR with their XOR, and these entries read the payload once and write
 * header + payload once. */

/* flags[i] of the reframe entries: emit nothing for frame i.  Honoured by
 * kmws_reframe_batch / kmws_unpack_reframe (and their _utf8 forms) only: kmws_encode_batch and
 * kmws_pack_headers ignore it, as they ignore every bit above KMWS_FLAG_MASK. */
#define KMWS_FLAG_SKIP 0x8000u

/* Workspace bytes for kmws_reframe_batch / kmws_unpack_reframe: at least
 * kmws_copy_workspace_size(n, dst_cap), plus 2 B per frame (the outgoing flags
 * kmws_unpack_reframe derives). */
size_t kmws_reframe_workspace_size(uint32_t n, uint64_t dst_cap);

/* descs[i] = {off, len, key}: key is the key the bytes src[off .. off+len) are
 * masked with now (0: plain); the descriptors need no order in src and payloads
 * may overlap, as for kmws_encode_batch.  flags[i] describes the outgoing
 * frame: header byte 0, KMWS_FLAG_MASK if it is masked, KMWS_FLAG_SKIP.
 * out_keys[i]: the outgoing key, used only when flags[i] & KMWS_FLAG_MASK; NULL:
 * every outgoing key is 0.  A frame that is not skipped writes
 * WSHandler::encodeFrameHeader of {flags[i] & 0x1FF, len, outgoing key}, then
 * the payload bytes src[off + j] ^ keybyte(descs[i].key, j) ^ (MASK ?
 * keybyte(outgoing key, j) : 0); frames lie back to back in dst.  A skipped
 * frame contributes no bytes -- wire_off[i + 1] == wire_off[i] -- and its
 * payload is never read (its off / len may point anywhere).  wire_off: n + 1
 * entries, wire_off[n] = the total.
 * Consequences: with every descs[i].key == 0 and no KMWS_FLAG_SKIP the output
 * is exactly kmws_encode_batch's; with the incoming key equal to the outgoing
 * key the payload is copied unchanged and the header carries the key.
 * The rest is kmws_encode_batch's contract: a total above dst_cap sets status
 * bit 1 and stores nothing; bit 4 on a look-back timeout; src and dst 16-byte
 * aligned and not overlapping; KMWS_ERR_INVALID_PARAM for a NULL wire_off or
 * workspace or, with frames, a NULL src / descs / flags / dst, and for a
 * misaligned src / dst; KMWS_ERR_BUFFER_TOO_SMALL for a workspace below
 * kmws_reframe_workspace_size(n, dst_cap); then KMWS_ERR_NOT_SUPPORTED without
 * a gfx950 device (no CPU fallback).  Stream-ordered, no host sync, no
 * allocation, kernel nodes only (capturable); the status word is cleared by a
 * kernel.  n == 0: KMWS_OK, wire_off[0] = 0. */
kmws_status kmws_reframe_batch(const uint8_t* src, const kmws_desc* descs, const uint16_t* flags,
                               const uint32_t* out_keys, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                               uint64_t* wire_off, void* workspace, size_t workspace_bytes, void* stream);

/* kmws_unpack_headers and kmws_reframe_batch fused: the descriptor-indexed
 * parse runs inside the scan, as in kmws_unpack_gather, and the payload pass
 * runs once.  out_desc, out_flags (keeps the incoming mask bit), out_err and
 * status bit 2 are exactly what kmws_unpack_gather writes.  Outgoing frame i
 * has the parsed header byte 0 -- FIN, RSV1-3 and the opcode are kept, so a
 * permessage-deflate message passes through -- and KMWS_FLAG_MASK iff out_mask
 * != 0; it is skipped iff its header had an error or bit `opcode` of
 * relay_opcodes is clear (0x0007: CONTINUE, TEXT and BINARY; 0xFFFF: everything
 * that parsed).  dst, wire_off and the status are exactly what
 * kmws_reframe_batch writes from those outgoing flags and out_desc on the same
 * wire.  The outgoing flags live in the workspace.  KMWS_ERR_INVALID_PARAM for
 * a bad mode, relay_opcodes > 0xFFFF, out_mask not 0 or 1; then the pointer and
 * alignment rules of kmws_unpack_gather (wire_off and workspace always; wire,
 * hdr_off, out_desc, dst with frames; wire and dst 16-byte aligned);
 * KMWS_ERR_BUFFER_TOO_SMALL; KMWS_ERR_NOT_SUPPORTED.  out_keys may be NULL
 * whatever out_mask is.  With status bit 2 some frames were dropped for header
 * errors: the caller fails those connections (out_err). */
kmws_status kmws_unpack_reframe(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n,
                                int mode, kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err,
                                uint32_t relay_opcodes, int out_mask, const uint32_t* out_keys,
                                uint8_t* dst, uint64_t dst_cap, uint64_t* wire_off,
                                void* workspace, size_t workspace_bytes, void* stream);

/* ---- unmask, re-encode and UTF-8 validation in one pass over the payload ----
 * A relay of text traffic must fail a connection that sends malformed text
 * (1007) and must not pass its bytes on.  kmws_utf8_validate(.., payload_masked
 * = 1, ..) on the incoming wire followed by kmws_unpack_reframe reads every
 * payload byte twice; these entries validate the words the reframe stores from
 * the registers that hold them.
 *
 * Workspace bytes: kmws_reframe_workspace_size(n, dst_cap) (rounded up to 256)
 * plus the validator's per-frame and per-stream arrays (about 12 B per frame,
 * 8 B per stream) -- not its tile plan. */
size_t kmws_reframe_utf8_workspace_size(uint32_t n, uint64_t dst_cap, uint32_t n_streams);

/* The two contracts composed.  dst, wire_off and the status word are exactly
 * what kmws_reframe_batch leaves for the same src / descs / flags / out_keys /
 * n / dst / dst_cap (the cap rule: total > dst_cap sets status bit 1 and stores
 * nothing; bit 4 on a look-back timeout; bytes of dst past wire_off[n] are
 * untouched); src is never written, the descriptors need no order in src and
 * may overlap, and a skipped frame's off / len are never used for an address.
 * out_utf8 (n bytes) and carry_out describe the messages as they are emitted: a
 * frame flagged KMWS_FLAG_SKIP is invisible to the check -- it gets
 * KMWS_UTF8_NOT_TEXT and does not touch the message state, like a control
 * frame, and its payload is never read.  Precisely, they are what
 * kmws_utf8_validate(dst, wire_off[n], D, F, n, 1, stream_first, n_streams,
 * carry_in, carry_out, ..) writes on the finished output wire, with, for an
 * emitted frame, D[i] = {wire_off[i] + its header's length, descs[i].len, the
 * outgoing key if flags[i] & KMWS_FLAG_MASK else 0} and F[i] = flags[i] & 0x1FF,
 * and for a skipped frame D[i] = {wire_off[i], 0, 0} and F[i] = 0x89 (a FIN
 * PING).  Text-ness comes from byte 0 of the outgoing flags.  The verdict is
 * advisory: a BAD message is reframed like any other, and the caller drops it
 * before dst goes to the sockets.  stream_first / carry_in / carry_out:
 * kmws_utf8_validate's; a malformed stream_first sets status bit 1 (nothing is
 * stored then).  With status bit 1 or 4 set out_utf8 / carry_out are not valid.
 * Stream-ordered, no host sync, no allocation, kernel nodes only (capturable);
 * the status word is cleared by a kernel.  KMWS_ERR_INVALID_PARAM for a NULL
 * required pointer (wire_off and workspace always; src, descs, flags, dst,
 * out_utf8 with frames), a misaligned src / dst, n or n_streams >= 2^31, NULL
 * stream_first with n_streams != 1, n_streams == 0 with frames; then
 * KMWS_ERR_BUFFER_TOO_SMALL; then KMWS_ERR_NOT_SUPPORTED without a gfx950
 * device (no CPU fallback).  n == 0: KMWS_OK, wire_off[0] = 0, carry_out =
 * carry_in. */
kmws_status kmws_reframe_utf8_batch(const uint8_t* src, const kmws_desc* descs, const uint16_t* flags,
                                    const uint32_t* out_keys, uint32_t n, uint8_t* dst, uint64_t dst_cap,
                                    uint64_t* wire_off,
                                    const uint32_t* stream_first, uint32_t n_streams,
                                    const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                    uint8_t* out_utf8, void* workspace, size_t workspace_bytes, void* stream);

/* kmws_unpack_reframe with the validation in its payload pass.  out_desc,
 * out_flags (required here), out_err, dst, wire_off and status bits 1, 2 and 4
 * are exactly as after kmws_unpack_reframe; out_utf8 and carry_out are exactly
 * kmws_reframe_utf8_batch's for the outgoing flags this call derives (the parsed
 * header byte 0, so incoming and outgoing text-ness agree).  A frame that is
 * not relayed -- an opcode outside relay_opcodes, or a header error -- is
 * skipped, hence invisible to the check: KMWS_UTF8_NOT_TEXT, the message state
 * untouched.  This differs from kmws_unpack_gather_utf8, which judges a frame
 * with a header error as the empty frame it becomes; here as there, look at
 * out_err (or status bit 2, with which out_utf8 / carry_out stay valid) before
 * out_utf8.  KMWS_ERR_INVALID_PARAM for a bad mode, relay_opcodes > 0xFFFF or
 * out_mask not 0 or 1 first; then kmws_reframe_utf8_batch's checks in its order
 * (wire, hdr_off, out_desc, out_flags, dst, out_utf8 with frames). */
kmws_status kmws_unpack_reframe_utf8(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n,
                                     int mode, kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err,
                                     uint32_t relay_opcodes, int out_mask, const uint32_t* out_keys,
                                     uint8_t* dst, uint64_t dst_cap, uint64_t* wire_off,
                                     const uint32_t* stream_first, uint32_t n_streams,
                                     const kmws_utf8_carry* carry_in, kmws_utf8_carry* carry_out,
                                     uint8_t* out_utf8, void* workspace, size_t workspace_bytes, void* stream);

/* ---- host-resident batches: pinned H2D -> kernel -> D2H pipeline ---- */
typedef struct kmws_pipeline kmws_pipeline;

/* depth slots (streams) of chunk_bytes device buffer each; chunks are cut on
 * frame boundaries with at most max_frames_per_chunk frames. */
kmws_pipeline* kmws_pipeline_create(int device, uint64_t chunk_bytes, uint32_t max_frames_per_chunk, int depth);
void           kmws_pipeline_destroy(kmws_pipeline* p);

/* Transfer mode: AUTO = chunked SDMA copies through device slots (H2D, kernel
 * and D2H on three streams, so both DMA directions run at once), except for a
 * pinned host_base (hipHostMalloc / hipHostRegister) spanning less than two
 * chunks, which gets one zero-copy launch (the kernel reads and writes host
 * memory over PCIe); COPY forces the chunked SDMA path; ZEROCOPY requires
 * pinned memory.  At most 3 slots are used at once whatever the depth. */
enum kmws_xfer { KMWS_XFER_AUTO = 0, KMWS_XFER_COPY = 1, KMWS_XFER_ZEROCOPY = 2 };
kmws_status kmws_pipeline_set_transfer(kmws_pipeline* p, int mode);

/* In-place unmask of frames that live in HOST memory (descs on the host,
 * offsets relative to host_base, sorted, within span).  Synchronous: returns
 * when every byte is back in host_base.  Only the frames' extents are written
 * back by the copy path; the zero-copy path rewrites their 16-B hulls.
 * Every descriptor is checked before anything is queued: unsorted, overlapping
 * or out-of-span frames return KMWS_ERR_INVALID_PARAM, a frame whose 16-B hull
 * exceeds chunk_bytes KMWS_ERR_BUFFER_TOO_SMALL, with host_base untouched; a
 * HIP failure mid-batch drains every queued copy before returning. */
kmws_status kmws_pipeline_unmask(kmws_pipeline* p, uint8_t* host_base, uint64_t span, const kmws_desc* descs,
                                 uint32_t n);

/* ---- pinned host memory for the loop rings ---- */

/* Page-locked host memory for the receive / send rings (kmws_rx_batch_attach_ring,
 * kmws_tx_batch_attach_ring): hipHostMalloc'ed, visible to `device`, so a
 * caller like kuma needs no HIP headers of its own.  NULL on failure. */
void* kmws_host_alloc(size_t bytes, int device);
void  kmws_host_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* KMWS_GPU_H */
