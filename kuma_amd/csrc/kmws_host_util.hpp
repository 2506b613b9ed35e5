// Host-side helpers shared by the decoder, the rx batch and the pipeline:
// device guard, pinned-memory detection and the pinned staging area whose
// payloads the unmask kernel processes in place over PCIe (zero-copy).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "kmws_common.hpp"
#include "kmws_gpu.h"
#include "kmws_utf8_rule.hpp"

namespace kmws {

// Switch to `dev` for the scope; restore the caller's current device on exit.
struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DevGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// Device-visible address of pinned host memory (hipHostMalloc / hipHostRegister),
// or nullptr for pageable memory.
inline void* device_view(void* host)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, host) != hipSuccess) {
        (void)hipGetLastError();  // clear the error left for pageable pointers
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, host, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return d;
}

inline size_t grow(size_t need, size_t have)
{
    size_t c = have ? have : (size_t)1 << 20;
    while (c < need) c *= 2;
    return c;
}

// A checked frame's view: slot = its verdict byte, lookback = the 24 bits
// before its first payload byte.
inline Utf8View checked_view(uint32_t slot, uint32_t lookback)
{
    return Utf8View{slot, (lookback & 0xFFFFFFu) | kUtf8Checked};
}

// Descriptors of one buffer, with a view beside each once one of them is
// checked: `views` stays empty until the first checked descriptor and is padded
// lazily, so it may be shorter than `descs` (the rest: unchecked).
struct DescList {
    std::vector<kmws_desc> descs;
    std::vector<Utf8View> views;
    void add(uint64_t off, uint32_t len, uint32_t key) { descs.push_back(kmws_desc{off, len, key}); }
    void add_checked(uint64_t off, uint32_t len, uint32_t key, uint32_t lookback, uint32_t slot)
    {
        views.resize(descs.size(), Utf8View{0u, 0u});
        add(off, len, key);
        views.push_back(checked_view(slot, lookback));
    }
    const Utf8View* views_or_null() const { return views.empty() ? nullptr : views.data(); }
    size_t size() const { return descs.size(); }
    bool empty() const { return descs.empty(); }
    void clear()
    {
        descs.clear();
        views.clear();
    }
};

// Descriptors that target a pinned buffer other than a stage's own area: a
// caller's chunk, or the ring attached to a batch.  Offsets are relative to
// `base` and must end within `span` bytes of it.  dv: the device view of base
// if the owner has it (a ring attached once), else launch() looks it up
// (hipPointerGetAttributes).  An empty list means "no extra".
struct ExtraBuf {
    uint8_t* base = nullptr;
    uint64_t span = 0;
    uint8_t* dv = nullptr;
    DescList list;
    // Is [p, p + n) inside the buffer?
    bool holds(const uint8_t* p, size_t n) const
    {
        return base && p >= base && n <= span && (uint64_t)(p - base) <= span - n;
    }
};

// A batch of payloads unmasked in place by the GPU.  Payloads are appended to
// a pinned host area (16-B aligned starts); launch() posts them as one job on
// the calling thread's slot of the resident worker when they fit one, else
// enqueues the pieces kernel on the pinned area itself (zero-copy over PCIe)
// on the stage's own stream and records its completion event; done() / wait()
// follow whichever ran; run() = launch() + wait.  An optional second
// batch of descriptors can target another pinned buffer (an ExtraBuf: a
// caller's pinned chunk, or its registered receive or send ring).  The
// asynchronous rx / tx batches keep one stage per generation in flight
// (kmws_decoder.cpp).
// UTF-8 check (kmws_decoder_set_utf8_check): a descriptor added with
// staged().add_checked, or an extra one whose view is checked, makes the job a checked
// one, with a view per descriptor and one verdict byte per checked frame
// (utf8_slot / utf8_bad) in the stage's pinned arrays.  It is posted to the
// resident worker when it has at most kResMaxDescs payloads and at most
// kResMaxBytesChecked (64 KiB: below the max_res_bytes of an unchecked job)
// bytes and the thread has a free and idle slot -- the grid's validating
// instantiation writes the stage's verdict bytes -- and otherwise, or when the
// worker withdraws it unrun, launches unmask_pieces_utf8_kernel with the same
// views, the host-read edge word per piece and the same verdict bytes.  A job
// without a checked frame goes exactly the way it went before.
// A stream a batch owns and its stages share; declared first in the batch so
// it is destroyed after every stage.
struct BatchStream {
    hipStream_t s = nullptr;
    int device = -1;
    kmws_status create(int dev)
    {
        device = dev;
        if (dev < 0 || kmws_device_count() <= dev) return KMWS_ERR_NOT_SUPPORTED;
        DevGuard g(dev);
        return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? KMWS_OK : KMWS_ERR_FAILED;
    }
    ~BatchStream()
    {
        if (!s) return;
        DevGuard g(device);
        (void)hipStreamSynchronize(s);
        (void)hipStreamDestroy(s);
    }
};

class PinnedStage {
public:
    ~PinnedStage() { release(); }

    // shared: a stream the owner keeps for all its stages (a batch's
    // generations), else the stage creates its own.  Creating a stream can
    // take milliseconds -- a loop iteration that needed a new stage stalled
    // for 2-3.5 ms (r05i/r05j loopback, rx_task_max) -- so the batches create
    // theirs once.
    kmws_status init(int device, hipStream_t shared = nullptr)
    {
        if (dev_ok_ < 0) {
            device_ = device;
            dev_ok_ = (device >= 0 && kmws_device_count() > device) ? 1 : 0;
        }
        if (!dev_ok_) return KMWS_ERR_NOT_SUPPORTED;
        if (!stream_) {
            DevGuard g(device_);
            if (shared) {
                stream_ = shared;
                own_stream_ = false;
            } else if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) {
                return KMWS_ERR_FAILED;
            }
            if (hipEventCreateWithFlags(&done_, hipEventDisableTiming) != hipSuccess) return KMWS_ERR_FAILED;
        }
        return KMWS_OK;
    }
    int device() const { return device_; }
    hipStream_t stream() const { return stream_; }

    // Allocates the pinned staging area and descriptor / piece arrays ahead
    // of use (hipHostMalloc can take milliseconds inside a loop iteration).
    kmws_status warm()
    {
        kmws_status st = reserve(64u << 10);
        if (st == KMWS_OK) st = ensure_host(kResMaxDescs, 4 * kResMaxDescs);
        return st;
    }

    // Room for `bytes` more payload bytes (plus alignment) without moving offsets.
    kmws_status reserve(size_t bytes)
    {
        const size_t need = len_ + 16 + bytes;
        if (need <= cap_) return KMWS_OK;
        DevGuard g(device_);
        const size_t c = grow(need, cap_);
        uint8_t* p = nullptr;
        if (hipHostMalloc(reinterpret_cast<void**>(&p), c, hipHostMallocDefault) != hipSuccess) return KMWS_ERR_FAILED;
        if (h_) {
            std::memcpy(p, h_, len_);
            (void)hipHostFree(h_);
        }
        h_ = p;
        dv_h_ = static_cast<uint8_t*>(device_view(h_));
        cap_ = c;
        return KMWS_OK;
    }
    size_t append(const uint8_t* p, size_t n)  // after reserve(n)
    {
        const size_t off = (len_ + 15) & ~(size_t)15;
        if (n) std::memcpy(h_ + off, p, n);
        len_ = off + n;
        return off;
    }
    // Room for n bytes at a 16-B aligned offset (after reserve(n)); the caller fills it.
    uint8_t* alloc(size_t n, size_t* off)
    {
        *off = (len_ + 15) & ~(size_t)15;
        len_ = *off + n;
        return h_ + *off;
    }
    uint8_t* data() { return h_; }
    // The staged descriptors.  add_checked: a checked frame's payload, slot =
    // its verdict byte (utf8_slot()); key 0: checked only, not stored.
    DescList& staged() { return own_; }
    // The next verdict byte of this job: one per checked, non-empty frame, staged or extra.
    uint32_t utf8_slot() { return n_slots_++; }
    // After wait(): the payload pass found a byte of the slot's frame that the rule rejects.
    bool utf8_bad(uint32_t slot) const { return h_verdict_ && slot < n_slots_ && slot < desc_cap_ && h_verdict_[slot] != 0; }
    size_t n_desc() const { return own_.size(); }
    void clear()
    {
        len_ = 0;
        own_.clear();
        n_slots_ = 0;
    }

    // Unmask every staged descriptor (and those of `extra` in its buffer), then
    // wait for the GPU: launch() + wait().
    kmws_status run(const ExtraBuf& extra = ExtraBuf())
    {
        kmws_status st = launch(extra, kResMaxBytes);
        if (st != KMWS_OK) return st;
        return wait();
    }

    // Has the last launch() finished?  (true when nothing was launched)
    bool done()
    {
        if (!launched_) return true;
        if (res_pending_) {
            const int r = resident_test(res_);
            if (r == 1) return true;
            if (r == 0) return false;
            res_pending_ = false;
            if (r != KMWS_ERR_NOT_SUPPORTED || launch_saved() != KMWS_OK) return true;  // wait() reports it
        }
        const hipError_t e = hipEventQuery(done_);
        if (e == hipErrorNotReady) return false;
        (void)hipGetLastError();
        return true;  // finished, or failed: wait() reports which
    }
    // A launched job: spins on the event for a time that grows with its bytes
    // (a loop thread waiting for a small job should not be parked and woken by
    // the runtime; a large one should not burn a core), then parks.
    kmws_status wait()
    {
        if (!launched_) return KMWS_OK;
        if (res_pending_) {
            res_pending_ = false;
            const kmws_status st = resident_wait(res_);
            if (st == KMWS_ERR_TIMEOUT) abandon();
            if (st != KMWS_ERR_NOT_SUPPORTED) {
                launched_ = false;
                return st;
            }
            const kmws_status ls = launch_saved();  // withdrawn, never run: launch it now
            if (ls != KMWS_OK) {
                launched_ = false;
                return ls;
            }
        }
        launched_ = false;
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t e = hipEventQuery(done_);
            if (e == hipSuccess) return KMWS_OK;
            if (e != hipErrorNotReady) {
                (void)hipGetLastError();
                return KMWS_ERR_FAILED;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(spin_us_)) break;
        }
        return hipEventSynchronize(done_) == hipSuccess ? KMWS_OK : KMWS_ERR_FAILED;
    }

    // Enqueue the unmask of every staged descriptor (and `extra`) without
    // waiting: a job of at most kResMaxDescs payloads and max_res_bytes bytes is
    // posted on the calling thread's slot of the device's resident worker (no
    // launch; kmws_resident.hip), anything else is launched on the stage's
    // stream (launch_unmask_pieces: no plan kernels, no copies, no status
    // read-back) with its completion event recorded.
    // max_res_bytes: the largest job posted on the worker (a synchronous run()
    // keeps kResMaxBytes: one workgroup is slower than a launch's many above it).
    // A view of extra.list checks its descriptor; a job with a checked frame,
    // staged or extra, is posted with its views and the zeroed verdict bytes if
    // it has at most min(max_res_bytes, kResMaxBytesChecked) bytes, else
    // launches the pieces kernel with the check.
    kmws_status launch(const ExtraBuf& extra = ExtraBuf(), uint64_t max_res_bytes = kResMaxBytes)
    {
        const std::vector<kmws_desc>& d2 = extra.list.descs;
        const std::vector<Utf8View>& v2 = extra.list.views;
        const size_t n1 = own_.size(), n2 = d2.size();
        if (n1 + n2 == 0) return KMWS_OK;
        if (launched_) return KMWS_ERR_INVALID_STATE;
        bool checked = !own_.views.empty();
        for (size_t i = 0; i < v2.size() && i < n2; ++i) checked |= (v2[i].w & kUtf8Checked) != 0u;
        for (const kmws_desc& x : d2)
            if (x.off + x.len > extra.span) return KMWS_ERR_INVALID_PARAM;
        uint8_t* dv2 = n2 && !extra.dv ? static_cast<uint8_t*>(device_view(extra.base)) : extra.dv;
        if (n2 && !dv2) return KMWS_ERR_INVALID_PARAM;  // must be pinned
        if (n1 && !dv_h_) return KMWS_ERR_FAILED;
        if (n1 + n2 <= (size_t)kResMaxDescs && (!checked || n_slots_ <= n1 + n2)) {
            // a checked job: its views, and the stage's verdict bytes zeroed
            ResidentCheck ck{};
            if (checked) {
                const kmws_status es = ensure_host(n1 + n2, 0);
                if (es != KMWS_OK) return es;
                own_.views.resize(n1, Utf8View{0u, 0u});
                std::memset(h_verdict_, 0, n1 + n2);
                ck = ResidentCheck{own_.views_or_null(), extra.list.views_or_null(), v2.size(), dv_verdict_,
                                   n_slots_, h_, extra.base};
            }
            const kmws_status st = resident_post(device_, own_.descs.data(), dv_h_, n1, n2 ? d2.data() : nullptr, dv2,
                                                 n2, &res_,
                                                 checked ? std::min(max_res_bytes, kResMaxBytesChecked) : max_res_bytes,
                                                 checked ? &ck : nullptr);
            if (st == KMWS_OK) {  // kept for a launch if the worker withdraws the job
                saved_ = extra;
                saved_.dv = dv2;
                saved_checked_ = checked;
                res_pending_ = true;
                launched_ = true;
                return KMWS_OK;
            }
            if (st != KMWS_ERR_NOT_SUPPORTED) return st;
        }
        return launch_kernels(extra, dv2, checked);
    }

private:
    // the call launch() makes, with the withdrawn job's own extra and check
    kmws_status launch_saved() { return launch_kernels(saved_, saved_.dv, saved_checked_); }

    // The device may still write the staging area (a resident job that timed
    // out) and, if the job was a checked one, the verdict bytes in the
    // descriptor allocation: both are left to the device -- never freed,
    // never reused.
    void abandon()
    {
        h_ = nullptr;
        dv_h_ = nullptr;
        cap_ = 0;
        len_ = 0;
        own_.clear();
        n_slots_ = 0;
        h_desc_ = nullptr;
        dv_desc_ = nullptr;
        h_view_ = dv_view_ = nullptr;
        h_verdict_ = dv_verdict_ = nullptr;
        desc_cap_ = 0;
    }

    // One record per piece of x, which is descriptor idx of its launch.  The
    // checked launch's record carries the four still-masked bytes before each
    // piece j >= 1 -- read here, from host memory, before anything is launched.
    static PieceRec* add_pieces(PieceRec* out, const uint8_t*, const kmws_desc& x, uint32_t idx)
    {
        for (uint64_t j = 0, c = piece_count(x.off, x.len); j < c; ++j) *out++ = PieceRec{idx, (uint32_t)j};
        return out;
    }
    static PieceRecEdge* add_pieces(PieceRecEdge* out, const uint8_t* host, const kmws_desc& x, uint32_t idx)
    {
        for (uint64_t j = 0, c = piece_count(x.off, x.len); j < c; ++j) {
            uint32_t edge = 0;
            if (j) std::memcpy(&edge, host + 16 * ((x.off >> 4) + j * kPieceWords) - 4, 4);
            *out++ = PieceRecEdge{idx, (uint32_t)j, edge};
        }
        return out;
    }
    // The pinned descriptor and piece arrays of a launch: the staged descriptors
    // with their pieces, then the extra ones rebased by delta onto eb, the extra
    // buffer's aligned base; their records index from the first extra descriptor
    // (the second launch gets dv_desc_ + n1).
    template <class Rec>
    void write_lists(const std::vector<kmws_desc>& d2, const uint8_t* eb, uint64_t delta)
    {
        const size_t n1 = own_.size();
        Rec* out = reinterpret_cast<Rec*>(h_piece_);
        if (n1) std::memcpy(h_desc_, own_.descs.data(), n1 * sizeof(kmws_desc));
        for (size_t i = 0; i < n1; ++i) out = add_pieces(out, h_, own_.descs[i], (uint32_t)i);
        for (size_t i = 0; i < d2.size(); ++i) {
            kmws_desc x = d2[i];
            x.off += delta;
            h_desc_[n1 + i] = x;
            out = add_pieces(out, eb, x, (uint32_t)i);
        }
    }

    // Launches the pieces kernel over the staged descriptors, then over the
    // extra ones (already checked by launch(); extra_dv: the buffer's device
    // view), and records the completion event.  checked: the kernel with the
    // UTF-8 check, which also gets a view per descriptor, the zeroed verdict
    // bytes and the edge word per piece; a job without a checked frame copies
    // and zeroes none of that.
    kmws_status launch_kernels(const ExtraBuf& extra, uint8_t* extra_dv, bool checked)
    {
        const std::vector<kmws_desc>& d2 = extra.list.descs;
        const std::vector<Utf8View>& v2 = extra.list.views;
        const size_t n1 = own_.size(), n2 = d2.size();
        DevGuard g(device_);
        // the extra buffer's 16-B aligned base, descriptors rebased onto it
        uint8_t* eb = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(extra.base) & ~(uintptr_t)15);
        const uint64_t delta = (uint64_t)(extra.base - eb);
        uint64_t p1 = 0, p2 = 0, bytes = 0;
        for (const kmws_desc& x : own_.descs) {
            p1 += piece_count(x.off, x.len);
            bytes += x.len;
        }
        for (const kmws_desc& x : d2) {
            p2 += piece_count(x.off + delta, x.len);
            bytes += x.len;
        }
        if (p1 + p2 > 0x7FFFFFFFull) return KMWS_ERR_INVALID_PARAM;
        kmws_status st = ensure_host(n1 + n2, p1 + p2);
        if (st != KMWS_OK) return st;
        if (checked) {
            if (n_slots_ > n1 + n2) return KMWS_ERR_INVALID_STATE;  // a slot without its descriptor
            own_.views.resize(n1, Utf8View{0u, 0u});
            if (n1) std::memcpy(h_view_, own_.views.data(), n1 * sizeof(Utf8View));
            for (size_t i = 0; i < n2; ++i) {  // a view whose slot is not below n_slots_ is unchecked
                Utf8View v = i < v2.size() ? v2[i] : Utf8View{0u, 0u};
                if (!(v.w & kUtf8Checked) || v.slot >= n_slots_) v = Utf8View{0u, 0u};
                h_view_[n1 + i] = v;
            }
            std::memset(h_verdict_, 0, n1 + n2);
            write_lists<PieceRecEdge>(d2, eb, delta);
        } else {
            write_lists<PieceRec>(d2, eb, delta);
        }
        // np pieces from piece q0 on, of the descriptors from d0 on, in the buffer at `base`
        auto go = [&](uint8_t* base, size_t d0, uint64_t q0, uint64_t np) {
            return checked ? launch_unmask_pieces_utf8(base, dv_desc_ + d0, dv_view_ + d0,
                                                       reinterpret_cast<PieceRecEdge*>(dv_piece_) + q0, (uint32_t)np,
                                                       dv_verdict_, stream_)
                           : launch_unmask_pieces(base, dv_desc_ + d0, dv_piece_ + q0, (uint32_t)np, stream_);
        };
        // the staging area's device view was taken when it was allocated; the
        // extra buffer goes by its aligned base's view (one mapping per allocation)
        if (p1) st = go(dv_h_, 0, 0, p1);
        if (st == KMWS_OK && p2) st = go(extra_dv - delta, n1, p1, p2);
        if (st != KMWS_OK) return st;
        if (hipEventRecord(done_, stream_) != hipSuccess) return KMWS_ERR_FAILED;
        // spin for about twice what the job should take (a launch's ~20 us, then
        // the payload over PCIe at ~8 GB/s each way), at least 1 ms -- a kernel
        // queued behind the resident grid on a shared hardware queue waits up
        // to its 1 ms lease, and a parked thread is woken milliseconds late
        // (loopback rx flushes of 2.6-5.1 ms with a 104 us spin, r05g) -- at
        // most 2 ms
        spin_us_ = std::min<uint64_t>(2000, std::max<uint64_t>(1000, 2 * (20 + (bytes >> 13))));
        launched_ = true;
        return KMWS_OK;
    }

    // Pinned descriptor and piece arrays (and their device views) for nd / np
    // entries.  Each allocation also holds what the checked launch adds for its
    // entries, so that the check brings no hipHostMalloc of its own into a loop
    // iteration: behind the c descriptors their c views and c verdict bytes; a
    // piece entry has room for the wider PieceRecEdge.
    kmws_status ensure_host(size_t nd, size_t np)
    {
        if (nd > desc_cap_) {
            const size_t c = std::max<size_t>(nd * 2, 1024);
            if (h_desc_) (void)hipHostFree(h_desc_);
            h_desc_ = nullptr;
            dv_desc_ = nullptr;
            h_view_ = dv_view_ = nullptr;
            h_verdict_ = dv_verdict_ = nullptr;
            desc_cap_ = 0;
            if (hipHostMalloc(reinterpret_cast<void**>(&h_desc_),
                              c * (sizeof(kmws_desc) + sizeof(Utf8View) + 1), hipHostMallocDefault) != hipSuccess)
                return KMWS_ERR_FAILED;
            dv_desc_ = static_cast<kmws_desc*>(device_view(h_desc_));
            if (!dv_desc_) return KMWS_ERR_FAILED;
            h_view_ = reinterpret_cast<Utf8View*>(h_desc_ + c);
            dv_view_ = reinterpret_cast<Utf8View*>(dv_desc_ + c);
            h_verdict_ = reinterpret_cast<uint8_t*>(h_view_ + c);
            dv_verdict_ = reinterpret_cast<uint8_t*>(dv_view_ + c);
            desc_cap_ = c;
        }
        if (np > piece_cap_) {
            const size_t c = std::max<size_t>(np * 2, 1024);
            if (h_piece_) (void)hipHostFree(h_piece_);
            h_piece_ = nullptr;
            dv_piece_ = nullptr;
            piece_cap_ = 0;
            static_assert(sizeof(PieceRecEdge) >= sizeof(PieceRec), "one array serves both launches");
            if (hipHostMalloc(reinterpret_cast<void**>(&h_piece_), c * sizeof(PieceRecEdge), hipHostMallocDefault) !=
                hipSuccess)
                return KMWS_ERR_FAILED;
            dv_piece_ = static_cast<PieceRec*>(device_view(h_piece_));
            if (!dv_piece_) return KMWS_ERR_FAILED;
            piece_cap_ = c;
        }
        return KMWS_OK;
    }
    void release()
    {
        if (launched_) (void)wait();  // nothing may outlive its pinned memory (a timed-out job's is abandoned)
        if (stream_ && own_stream_) (void)hipStreamSynchronize(stream_);
        if (done_) (void)hipEventDestroy(done_);
        if (h_) (void)hipHostFree(h_);
        if (h_desc_) (void)hipHostFree(h_desc_);
        if (h_piece_) (void)hipHostFree(h_piece_);
        if (stream_ && own_stream_) (void)hipStreamDestroy(stream_);
    }

    int device_ = 0;
    int dev_ok_ = -1;
    hipStream_t stream_ = nullptr;
    bool own_stream_ = true;
    hipEvent_t done_ = nullptr;
    bool launched_ = false;
    bool res_pending_ = false;  // launched_ on the resident worker: res_ says which job
    ResidentJob res_;
    ExtraBuf saved_;              // a copy of a resident job's extra, for launch_saved()
    bool saved_checked_ = false;  // ... and its check
    uint64_t spin_us_ = 1000;
    uint8_t* h_ = nullptr;
    uint8_t* dv_h_ = nullptr;
    size_t cap_ = 0, len_ = 0;
    DescList own_;          // the staged descriptors: offsets into h_
    uint32_t n_slots_ = 0;  // verdict bytes handed out (utf8_slot)
    kmws_desc* h_desc_ = nullptr;   // pinned, read by the kernel over PCIe
    kmws_desc* dv_desc_ = nullptr;  // its device view
    Utf8View* h_view_ = nullptr;    // behind the descriptors, in their allocation
    Utf8View* dv_view_ = nullptr;
    uint8_t* h_verdict_ = nullptr;  // behind the views: written by the checked launch, read after wait()
    uint8_t* dv_verdict_ = nullptr;
    size_t desc_cap_ = 0;
    PieceRec* h_piece_ = nullptr;
    PieceRec* dv_piece_ = nullptr;
    size_t piece_cap_ = 0;
};

}  // namespace kmws
