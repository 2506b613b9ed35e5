// Resident unmask worker: the synchronous host entries without a kernel launch
// per call, concurrent across the process's event-loop threads.
//
// kuma calls WSHandler::handleData once per <= 64 KiB socket read
// (TcpConnection.cpp:229-233 -> WebSocketImpl.cpp:225-246) and
// WSHandler::handleDataMask once per send (WebSocketImpl.cpp:388, :414), and
// expects the payload unmasked when the call returns -- on every loop thread
// (10 in kuma's test client, test/client/main.cpp:20; 5 in its server,
// test/server/main.cpp:22).  A stream launch plus an event wait costs 13-15 us
// per call, about what kuma's byte loop (WSHandler.cpp:303-310) spends on a
// whole 64 KiB read.  Here ONE grid of kResSlots workgroups (1024 lanes each)
// stays resident per device, on one greatest-priority stream: workgroup b
// serves mailbox slot b, and a host thread claims a slot once (lock-free) and
// keeps it until it exits.  Each slot is polled from pinned host memory by its
// own workgroup: the thread writes a job (up to kResMaxDescs payloads, each a
// device-visible address, a length and a key) and bumps the slot's job
// number; the workgroup sees it over PCIe, unmasks every payload in place
// there (zero-copy, 4 x 16-byte words per lane in flight: 64 KiB per round),
// makes its stores visible system-wide and writes the job number back; the
// thread spins on that word.  No launch, no completion signal, no interrupt,
// no lock: threads on different slots run their jobs at the same time.  A
// thread that finds no free slot launches on its own stream instead; it never
// waits for another thread.  (One grid, not a worker per thread: two workers'
// greatest-priority streams shared a hardware queue, so one thread's job
// waited for the other's worker to leave -- round 4, r04x.)
//
// The grid exits by itself after kResIdleUs (200 us) without a job in any
// slot, after a lease of kResLeaseUs (1 ms) however busy it is, and a
// workgroup leaves on its slot's quit bit (process exit; a job past its
// timeout): every wave reaches the exit, the grid drains, and a host thread
// that stops feeding never leaves a kernel behind.  The next job relaunches
// it.  The stream is non-blocking and of the greatest priority, so work on
// other streams -- the legacy default stream included -- does not queue behind
// it, and the lease bounds the wait of any kernel that still shares its
// hardware queue (tests/test_gpu_decoder.py).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "kmws_bench.h"
#include "kmws_host_util.hpp"
#include "kmws_utf8_dev.hpp"
#include "kmws_resident_proto.hpp"

namespace kmws {

// Jobs of up to this many 16-byte words store write-through (sc0 sc1) and end
// without a release; larger ones store into the L2 and end with one
// system-scope release (a buffer_wbl2 of the XCD's L2) -- unless a device
// batch of this library is running on the device (kmws::note_device_batch):
// then every job writes through.  A release per job at a million small jobs a
// second slowed a device batch beside the grid (tools/grid_interference.cpp),
// and with 64 KiB jobs 1.36x against 1.11x written through (r06az); write-
// through stores of 64 KiB generations halved 8 loopback connections' decode
// (18.6 -> 8.6-10.9 GiB/s, r06an-ap).  The thread decides (kWriteThroughBit).
constexpr int kResWriteThroughWords = 1024;
// Idle exit: short.  The runtime maps streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES, 4 on the box), so a kernel launched on a stream that
// shares the worker's queue waits until the worker leaves; and
// hipDeviceSynchronize (torch.cuda.synchronize) waits for every stream, the
// worker's included (measured: a device synchronize behind a 50 ms-idle worker
// took 50 ms; the loopback "gpu" mode, whose batches keep several streams, fell
// from 2.0 to 0.57 GiB/s with a 5 ms idle).  A loop thread under load feeds far
// more often than this; a worker that idled out costs one launch at the next
// job, the price of every call without it.
constexpr uint32_t kResIdleUs = 200;
// Lease: an incarnation also leaves after kResLeaseUs of life however busy it
// is, before it takes the next job (the host relaunches it for that job).  A
// thread that feeds back to back would otherwise keep the worker resident for
// good, and a kernel on another stream that shares its hardware queue would
// wait for as long (measured: up to 6.9 s behind a feeder thread).  The
// relaunch it costs (~10-15 us) is spread over the ~100 jobs of one lease.
constexpr uint32_t kResLeaseUs = 1000;
// A job not done after kResTimeoutMs is withdrawn: the slot's quit bit asks
// its workgroup to leave, and the thread waits up to kResDrainMs more for it.
// Only when the workgroup has left (or finished the job) does the call return
// without KMWS_ERR_TIMEOUT -- nothing writes the payloads after that.  The
// test build shortens both (kuma_amd/build.py).
#ifndef KMWS_RESIDENT_TIMEOUT_MS
#define KMWS_RESIDENT_TIMEOUT_MS 2000
#endif
#ifndef KMWS_RESIDENT_DRAIN_MS
#define KMWS_RESIDENT_DRAIN_MS 2000
#endif
// A job whose workgroup left while the rest of the grid still runs (it is
// closing, or another workgroup is stuck in a job) is withdrawn after this long
// and launched by the caller.
constexpr uint32_t kResOrphanUs = 200;

static inline void cpu_relax()
{
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    __builtin_ia32_pause();
#endif
}

// What a checked job adds (ResSlot::view, ::verdict): per payload its view
// word and its host address (the edge words are read there), and the device
// view of the verdict bytes.
struct ResCheckArgs {
    uint64_t view[kResMaxDescs];
    const uint8_t* host[kResMaxDescs];
    uint64_t verdict;
};

// Loads of host-written words bypass every cache (and are never scalar loads).
__device__ __forceinline__ uint64_t ld_sys(const uint64_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Write-through (sc0 sc1: system scope) stores of a small job's payload
// bytes (kResWriteThroughWords).  Complete -- written through to host memory
// -- once the storing wave's vmcnt drains, so the done word needs no release:
// a system-scope release is a buffer_wbl2 of the whole XCD L2, which at a
// million small jobs a second stalled a device batch running beside the grid
// (tools/grid_interference.cpp).  A lane's four words go in ONE asm
// statement: the compiler waits for every access in flight before an inline
// asm, so four statements made each store wait for the one before.  Flat
// stores: a lane with nothing to store aims its words at its own 16 bytes of
// LDS (no memory traffic).  8-byte stores the compiler could count instead
// wrote half of every 16 bytes per instruction and ran 10x slower (r06ao).
__device__ __forceinline__ void st_sys16x4(uint64_t a0, u32x4 v0, uint64_t a1, u32x4 v1, uint64_t a2, u32x4 v2,
                                           uint64_t a3, u32x4 v3)
{
    asm volatile(
        "flat_store_dwordx4 %0, %1 sc0 sc1\n\t"
        "flat_store_dwordx4 %2, %3 sc0 sc1\n\t"
        "flat_store_dwordx4 %4, %5 sc0 sc1\n\t"
        "flat_store_dwordx4 %6, %7 sc0 sc1\n\t"
        "s_nop 1" ::"v"(a0),
        "v"(v0), "v"(a1), "v"(v1), "v"(a2), "v"(v2), "v"(a3), "v"(v3)
        : "memory");
}
// A small job's hull edge bytes, written through: stores the compiler counts
// (no wait between them).
__device__ __forceinline__ void st_sys1(uint64_t a, uint32_t v)
{
    __hip_atomic_store(reinterpret_cast<__attribute__((address_space(1))) uint8_t*>(a), (uint8_t)v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// ResCtl lives in uncached device memory (ResidentWorker::init), so a plain
// load of a word other XCDs update is never served stale from this XCD's L2
// (a read-modify-write would be coherent too, but 64 workgroups doing one on
// the same word every fourth poll serialized at the atomic unit).
__device__ __forceinline__ uint64_t ld_agent(const uint64_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Lane 0's value in every lane (each half through uint32_t: readfirstlane is signed).
__device__ __forceinline__ uint64_t first_lane64(uint64_t v)
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32)) << 32;
}
// One descriptor of the slot, read after the job word was seen.
__device__ __forceinline__ ResDesc load_desc(const ResDesc* d)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(d);
    const uint64_t lo = ld_sys(q), hi = ld_sys(q + 1);  // each half one 8-byte load
    return untag_desc(ResDesc{lo, (uint32_t)hi, (uint32_t)(hi >> 32)});
}
// Wave 0's state from poll to poll.  (The order of the fields is the one that
// keeps the kernel's registers where they were: profiles/p12_resident_isa.txt.)
struct Wave0 {
    bool full;       // poll the descriptors too
    bool idle;       // counted in ctl->idle
    uint64_t last;   // job seen last
    uint64_t t_act;  // this slot's latest job
    uint32_t why;    // the exit reason (ResCtl::why, ResExit)
};

// nslots x kResParts workgroups (slots 0 .. nslots - 1: those claimed when
// the incarnation was launched), persistent until idle: workgroup blockIdx.x
// serves part p = blockIdx.x / nslots of slot (blockIdx.x - p) mod nslots, i.e.
// part p of slot s sits at p * nslots + (s + p) mod nslots.  Workgroups are
// dealt to the 8 XCDs by blockIdx.x mod 8, so slot s's part 0 (all a small job
// uses) is on XCD s mod 8 and its four parts on four different XCDs: with
// blockIdx.x mod nslots as the slot, 8 or 16 slots put a slot's parts on one
// XCD, and slot-major numbering put every part 0 on XCDs 0 and 4 (16 threads'
// 4 KiB masks 2.2 -> 1.6 M calls/s, r05bk; the diagonal keeps 2.2 M and gives 8
// loopback connections' one-end runs 0-10 % more, r05bl).  A job's hull words are split evenly over its parts;
// each part polls the slot's job word itself -- no hand-off between
// workgroups -- runs its words and writes its own done word.  `inc` = this
// incarnation's number (from 1); `exit_base` = the workgroups of every
// earlier incarnation (the exit counter's value once they all left).
//
// kCheck: the validating instantiation.  It runs unchecked jobs as <false>
// does and validates the text payloads of a checked one (kCheckBit) on the
// unmasked words it holds before they leave its registers: the rule of
// kmws_utf8_dev.hpp on each word, with the dword before the word from the lane
// below, from the wave below and the stripe before through LDS (s_row, behind
// one barrier), from the host-read edge word at a part's first word and from
// the view at a payload's first byte.  A checked part is one round of at most
// kResBlock * kResWords words -- the host posts no checked job with a larger
// one (ResidentWorker::post) -- so nothing is carried from round to round.  <false> is the kernel without any of it:
// a process that never turns the check on runs that one, at its footprint.
template <bool kCheck>
__global__ void __launch_bounds__(kResBlock) resident_unmask_kernel(ResMailbox* mb, ResCtl* ctl, uint64_t inc,
                                                                    uint32_t nslots, uint64_t exit_base,
                                                                    uint64_t idle_ticks, uint64_t lease_ticks)
{
    // (kCheck) per payload: its view word; per stripe and wave: the last
    // unmasked dword of the wave's 64 words; the verdict bytes' address
    __shared__ uint64_t s_view[kCheck ? kResMaxDescs : 1];
    __shared__ uint32_t s_row[kResWords][kResBlock / 64];
    __shared__ uint64_t s_verdict;
    __shared__ ResDesc s_d[kResMaxDescs];
    __shared__ uint32_t s_pre[kResMaxDescs + 1];  // word prefix over the payload hulls
    __shared__ uint64_t s_cmd;
    __shared__ uint32_t s_have;  // descriptors taken from the poll
    __shared__ u32x4 s_sink[kResBlock];  // per lane: where a lane with no whole word stores its words
    const int t = threadIdx.x;
    const uint32_t part = blockIdx.x / nslots;
    ResSlot* sl = &mb->slot[(blockIdx.x % nslots + nslots - part % nslots) % nslots];
    const uint64_t born = wall_clock64();
    const uint64_t my_sink = reinterpret_cast<uint64_t>(static_cast<void*>(&s_sink[t]));  // a flat (LDS) address
    // lane l <= kPollDescs of wave 0 of part 0 polls bytes [16 l, 16 l + 16)
    // of the slot: the job word (lane 0) and descriptor slot l - 1; other
    // parts, and part 0 while the slot is unclaimed, load the word only (one
    // request)
    const uint64_t* pw0 = &sl->word;
    const uint64_t* pw = pw0 + 2 * (t <= kPollDescs ? t : 0);
    // Idle exit without comparing clocks across workgroups: a workgroup whose
    // slot has had no job for idle_ticks counts itself in ctl->idle (and out
    // again at the slot's next job, whichever part it is for); the one whose
    // count completes the grid closes it.  Before, each compared its clock with
    // a device-wide "last job" time other workgroups wrote, and under load read
    // it stale or skewed: 16 busy threads' grids closed as idle every ~0.3 ms
    // (r05as / r05at: 650-1,199 idle decisions in 25 ms; 1.26 M calls/s).
    Wave0 s{part == 0, false, 0, born, kExitLease};
    if (t < 64) s.last = ld_sys(&sl->done[part]);
    for (;;) {
        if (t < 64) {  // wave 0, uniform control flow
            uint64_t cmd = 0, v0 = 0, v1 = 0;
            bool polled_full = false;
            for (uint32_t it = 0;; ++it) {
                const uint64_t now = wall_clock64();
                const uint64_t* a = s.full ? pw : pw0;
                v0 = ld_sys(a);
                v1 = ld_sys(a + 1);
                // with the word's loads in flight: is the grid leaving (idle;
                // every 4th poll) or asked to (a thread claimed a slot it does
                // not serve, and the relaunch will; every 16th poll -- every 4th,
                // 64 workgroups reading that one host word slowed 16 threads'
                // jobs to 1.4 M/s at an 11 us median, against 2.1 M/s at 6.5 us,
                // r05av)?  A posted job waits for the relaunch, as at the lease.
                uint64_t closing = 0, resize = 0;
                if ((it & 3u) == 0) closing = ld_agent(&ctl->closing);
                if ((it & 15u) == 0) resize = ld_sys(&mb->resize);
                if ((uint64_t)(now - born) > lease_ticks || closing >= inc || resize >= inc) {
                    s.why = closing >= inc ? kExitClosing : resize >= inc ? kExitResize : kExitLease;
                    cmd = 0;
                    break;
                }
                polled_full = s.full;
                const uint64_t w = first_lane64(v0);  // lane 0's job word
                if (job_quit(w)) {  // this slot only: the rest of the grid serves on
                    s.why = kExitQuit;
                    break;
                }
                const uint64_t job = job_number(w);
                if (job != s.last) {  // a job on this slot: activity, whichever part it is for
                    s.t_act = now;
                    if (s.idle) {
                        if (t == 0) __hip_atomic_fetch_sub(&ctl->idle, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s.idle = false;
                    }
                    const uint32_t parts = job_parts(w);
                    if (part >= parts || (w & kCancelBit)) {
                        s.last = job;  // not this workgroup's (no done word: nobody waits for it)
                        continue;
                    }
                    cmd = w;
                    break;
                }
                const bool claimed = job_claimed(w) != 0;
                s.full = part == 0 && claimed;
                if (!s.idle && (uint64_t)(now - s.t_act) > idle_ticks) {  // idle here: counted
                    uint64_t before = 0;
                    if (t == 0) before = __hip_atomic_fetch_add(&ctl->idle, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    before = first_lane64(before);
                    s.idle = true;
                    if (before + 1 >= gridDim.x) {  // every workgroup idle: the grid leaves
                        if (t == 0) __hip_atomic_fetch_max(&ctl->closing, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s.why = kExitIdle;
                        break;
                    }
                }
                if (claimed) __builtin_amdgcn_s_sleep(2);
                else __builtin_amdgcn_s_sleep(127);  // ~4 us: an unclaimed slot gets a job rarely
            }
            uint32_t have = 0;
            if (cmd) {
                const uint32_t nd = job_count(cmd);
                const ResDesc x = ResDesc{v0, (uint32_t)v1, (uint32_t)(v1 >> 32)};
                const bool mine = polled_full && t >= 1 && t <= (int)nd && t <= kPollDescs;
                const bool ok = desc_tagged(x, job_number(cmd));
                if (mine && ok) s_d[t - 1] = untag_desc(x);
                // every descriptor of the job came with the word: no second round trip
                const uint64_t bad = __ballot(mine && !ok);
                have = polled_full && nd <= (uint32_t)kPollDescs && bad == 0 ? nd : 0u;
                // acquire at system scope (the CU's vector L1 and the L2): the
                // payloads (and descriptors) the host wrote before the job word
                // are read fresh; the other waves load after the barrier below
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                if constexpr (kCheck) {
                    // lane 0's second half is the word beside the job word: the
                    // verdict bytes' address, read again if its tag is stale
                    if (t == 0 && job_checked(cmd)) {
                        if (!verdict_tagged(v1, cmd)) v1 = ld_sys(pw0 + 1);
                        s_verdict = untag_verdict(v1);
                    }
                }
            }
            if (t == 0) {
                s_cmd = cmd;
                s_have = have;
            }
        }
        __syncthreads();
        const uint64_t cmd = s_cmd;
        if (cmd == 0) break;  // every wave leaves together
        const uint32_t nd = job_count(cmd);
        const uint32_t n = nd < (uint32_t)kResMaxDescs ? nd : (uint32_t)kResMaxDescs;
        if (s_have == 0 && t < (int)n) s_d[t] = load_desc(&sl->desc[t]);
        __syncthreads();
#ifdef KMWS_TEST_RESIDENT_STALL_KEY
        // test build only (kuma_amd/build.py): a job whose first payload's key
        // has these upper 24 bits stalls the workgroup for (key & 0xFF) x 10 ms,
        // then is dropped if its thread withdrew it meanwhile (the quit bit)
        if ((s_d[0].key & 0xFFFFFF00u) == (uint32_t)(KMWS_TEST_RESIDENT_STALL_KEY)) {
            const uint64_t t0 = wall_clock64(), ticks = lease_ticks / kResLeaseUs * 10000u * (s_d[0].key & 0xFFu);
            while ((uint64_t)(wall_clock64() - t0) < ticks) __builtin_amdgcn_s_sleep(127);
            if (t == 0 && (ld_sys(pw0) & kQuitBit)) s_cmd = 0;
            __syncthreads();
            if (s_cmd == 0) {
                s.why = kExitQuit;  // gone on its quit bit
                break;
            }
        }
#endif
        if (t == 0) {
            uint32_t w = 0;
            for (uint32_t i = 0; i < n; ++i) {
                s_pre[i] = w;
                w += hull_words(s_d[i].addr, s_d[i].len);
            }
            s_pre[n] = w;
        }
        __syncthreads();
        const bool wt = job_write_through(cmd) != 0;
        const PartRange mine = part_range(s_pre[n], part, job_parts(cmd));  // this part's words
        const uint32_t we = mine.end;
        // a checked part is one round with a barrier in it: every wave runs it
        const bool chk = kCheck && job_checked(cmd) != 0;
        for (uint32_t w0 = mine.begin; w0 < we; w0 += kResBlock * kResWords) {
            if (!chk && w0 + (uint32_t)(t & ~63) >= we) break;  // nothing left for this wave (uniform)
            u32x4 v[kResWords];
            uint32_t di[kResWords];
            // (checked) the views, one per lane, and this part's edge word:
            // loads that fly with the payload's
            uint64_t vw = 0, eg = 0;
            if constexpr (kCheck) {
                if (chk) {
                    if (t < (int)n) vw = ld_sys(&sl->view[t]);
                    if (t == 0) eg = ld_sys(&sl->edge[part]);
                }
            }
#pragma unroll
            for (int i = 0; i < kResWords; ++i) {
                // a lane past the part's end loads nothing (clamped to the
                // part's last word, many waves reading one host word stalled
                // the grid: 4 KiB jobs ran at 48 us, r06ao; a load from its
                // LDS sink instead cost a device batch beside the grid 1.08x
                // against 1.02x, r06ay).  One asm statement takes every store,
                // so the compiler's wait for these loads costs nothing more.
                const uint32_t w = w0 + t + kResBlock * i;
                uint32_t lo = 0, hi = n;  // last payload whose first word is <= w
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_pre[mid] <= w) lo = mid; else hi = mid;
                }
                di[i] = lo;
                const ResDesc x = s_d[lo];
                v[i] = u32x4{0, 0, 0, 0};
                if (w < we) v[i] = *reinterpret_cast<const u32x4*>(word_addr(x, w, s_pre[lo]));
            }
            // each word XORed with its payload's rotated key (the loads' registers
            // free from here: fewer live VGPRs leave more of each SIMD to a device
            // batch sharing the CU -- 96 against 82 cost that batch 1.07-1.08x
            // against 1.02x, r06bq)
            u32x4 sv[kResWords];
            uint64_t sa[kResWords];
            uint32_t edge = 0;  // bit i: word i is a hull's edge word of this part
#pragma unroll
            for (int i = 0; i < kResWords; ++i) {
                const uint32_t w = w0 + t + kResBlock * i;
                const ResDesc x = s_d[di[i]];
                const uint64_t a = word_addr(x, w, s_pre[di[i]]);
                sv[i] = v[i] ^ rot_key(x.key, x.addr);
                sa[i] = a;
                // no short-circuit: with `&&` the compiler (ROCm 7.2, gfx950)
                // branched around the descriptor's length and lost the sink
                // for the last word of a payload on word 0 -- it stored the
                // whole word, over the next frame's header (r06ap)
                // (a checked job stores nothing to a payload whose key is 0: a
                // CLIENT-mode decoder's unmasked frames are only validated)
                const bool in = (w < we) & !(chk & (x.key == 0u)),
                           whole = in & (a >= x.addr) & (a + 16 <= x.addr + x.len);
                edge |= (uint32_t)(in & !whole) << i;
                if (wt) sa[i] = whole ? a : my_sink;
                else if (whole) *reinterpret_cast<u32x4*>(a) = sv[i];  // into the L2 (the release follows)
            }
            // write-through: the four words in one asm statement
            static_assert(kResWords == 4, "st_sys16x4 stores four words");
            if (wt) st_sys16x4(sa[0], sv[0], sa[1], sv[1], sa[2], sv[2], sa[3], sv[3]);
            // a hull's edge words: this payload's bytes only
#pragma unroll
            for (int i = 0; i < kResWords; ++i) {
                if (!(edge >> i & 1u)) continue;
                const ResDesc x = s_d[di[i]];
                const uint64_t a = sa[i] == my_sink ? word_addr(x, w0 + t + kResBlock * i, s_pre[di[i]]) : sa[i];
                const uint64_t end = x.addr + x.len;
                const uint64_t lo = a > x.addr ? a : x.addr, hi = a + 16 < end ? a + 16 : end;
                for (uint64_t q = lo; q < hi; ++q) {
                    const uint32_t b = (uint32_t)(q - a);
                    const uint32_t dw = (b & 8u) ? ((b & 4u) ? sv[i].w : sv[i].z) : ((b & 4u) ? sv[i].y : sv[i].x);
                    const uint32_t o = dw >> (8 * (b & 3u));
                    if (wt) st_sys1(q, o);
                    else *reinterpret_cast<uint8_t*>(q) = (uint8_t)o;
                }
            }
            if constexpr (kCheck) {
                if (chk) {  // block-uniform
                    constexpr int kWaves = kResBlock / 64;
                    const int lane = t & 63, wave = t >> 6;
                    uint32_t(*row)[kWaves] = s_row;
                    if (t < (int)n) s_view[t] = vw;
                    if (lane == 63) {
#pragma unroll
                        for (int i = 0; i < kResWords; ++i) row[i][wave] = sv[i].w;
                    }
                    __syncthreads();
                    // the dword before the part's first word, unmasked: its edge
                    // word.  Like every look-back below it is used only where it
                    // belongs to the word's own payload (word_bad): its key phase
                    // is that word's.
                    uint32_t first = 0;
                    if (t == 0) first = (uint32_t)eg ^ rot_key(s_d[di[0]].key, s_d[di[0]].addr);
#pragma unroll
                    for (int i = 0; i < kResWords; ++i) {
                        const uint32_t w = w0 + t + kResBlock * i;
                        const uint32_t up = __shfl_up(sv[i].w, 1);
                        uint32_t prev = up;
                        if (lane == 0) prev = wave ? row[i][wave - 1] : (i ? row[i ? i - 1 : 0][kWaves - 1] : first);
                        const ResDesc x = s_d[di[i]];
                        const uint64_t view = s_view[di[i]];
                        const uint64_t a = word_addr(x, w, s_pre[di[i]]);
                        bool bad = false;
                        if (w < we && (view & kUtf8Checked))
                            bad = plain_word_frame_bad(sv[i], prev, a, x.addr, x.addr + x.len, (uint32_t)view);
                        // a rejected byte: the frame's verdict byte, written
                        // through, by one lane per wave and payload
                        uint64_t m = __ballot(bad);
                        while (m) {
                            const int leader = __ffsll((long long)m) - 1;
                            const uint32_t ld = (uint32_t)__shfl((int)di[i], leader);
                            if (lane == leader) st_sys1(s_verdict + (view >> 32), 1u);
                            m &= ~__ballot(bad && di[i] == ld);
                        }
                    }
                }
            }
        }
        // every wave waits for its own stores, then ONE lane writes the
        // part's done word: a small job's stores were written through (in
        // host memory once vmcnt drains), so no release; a large job's sit in
        // the L2 and that lane's release writes them back (one release: in all
        // 16 waves it cost 2.7 us more per 64 KiB job, tools/zc_probe.hip,
        // profiles/r05n_zc_probe.jsonl)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) {
            if (wt) __hip_atomic_store(&sl->done[part], job_number(cmd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else __hip_atomic_store(&sl->done[part], job_number(cmd), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (t < 64) {
            s.last = job_number(cmd);
            s.t_act = wall_clock64();  // the slot was busy until now (a long job is not idle time)
        }
    }
    if (t == 0) {
        __hip_atomic_fetch_add(&ctl->why[s.why < kResExitReasons ? s.why : 0], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s.why == kExitQuit && !s.idle) {  // gone on its quit bit: idle for the rest of the incarnation
            const uint64_t b = __hip_atomic_fetch_add(&ctl->idle, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (b + 1 >= gridDim.x) __hip_atomic_fetch_max(&ctl->closing, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(&sl->gone[part], inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint64_t before = __hip_atomic_fetch_add(&ctl->exits, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1 == exit_base + gridDim.x) {  // the grid's last workgroup: the next starts with none idle
            (void)__hip_atomic_exchange(&ctl->idle, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&mb->exited, inc, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

namespace {

void quit_all_workers();

template <class T>
T ld_acq(const T* p)
{
    return __atomic_load_n(p, __ATOMIC_ACQUIRE);
}

using Clock = std::chrono::steady_clock;

// A worker's event counts, behind the extern "C" counter entries: relaxed adds and reads.
struct Counters {
    // kUnownedPosts: posts refused, the caller did not hold the slot; kWtJobs, kReleasedJobs: jobs posted by
    // kind (kWriteThroughBit); kLatePosts: jobs asked for after the thread gave its slots back (launched);
    // kDrained: releases that first waited for the slot's last job
    enum Id { kTimeouts, kWithdrawn, kUnownedPosts, kWtJobs, kReleasedJobs, kLatePosts, kDrained, kVariantSwitches, kCount };
    void add(Id i) { __atomic_fetch_add(&v[i], 1, __ATOMIC_RELAXED); }
    uint64_t get(Id i) const { return __atomic_load_n(&v[i], __ATOMIC_RELAXED); }
    uint64_t v[kCount] = {};
};
// A part of a job: finished; not finished and its workgroup has left the grid
// (nobody will run it there); or still held by a workgroup that may run it.
enum class Part { kFinished, kLeft, kHeld };

// One per device, shared by every host thread.  Slots are claimed with one
// atomic on a bit mask; a job on a slot needs no lock (the slot's thread is
// its only writer).  launch_mu_ is taken only to relaunch the grid or to
// withdraw a job no workgroup can take any more.  Never freed: releasing
// pinned memory from a static destructor can run after the HIP runtime was
// torn down.  At process exit an atexit handler -- registered after the HIP
// runtime's own, so it runs before the runtime's teardown -- asks every
// workgroup to quit and waits (bounded) until the grid has exited.
class ResidentWorker {
public:
    explicit ResidentWorker(int device) : device_(device) {}

    // A free slot for the calling thread (its owner token `me`, never 0), or
    // -1 (all taken, or unusable).
    int claim(uint64_t me)
    {
        if (!usable()) return -1;
        uint32_t m = ld_acq(&claimed_);
        for (;;) {
            if (m == 0xFFFFFFFFu >> (32 - kResSlots)) return -1;
            const int b = __builtin_ctz(~m);
            if (__atomic_compare_exchange_n(&claimed_, &m, m | (1u << b), false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
                __atomic_store_n(&hs_[b].owner, me, __ATOMIC_RELEASE);
                // the workgroup polls the descriptors from now on (no job: same number)
                __atomic_fetch_or(&mb_->slot[b].word, kClaimedBit, __ATOMIC_RELEASE);
                // a running incarnation without this slot's workgroups is asked
                // to leave; the next job relaunches a grid that serves it
                const uint64_t cur = ld_acq(&inc_);
                if (cur && (uint32_t)b >= ld_acq(&nslots_)) request_resize(cur);
                return b;
            }
        }
    }
    // The thread `me` gives slot b back (thread exit, or it switched the worker
    // off).  Its last job -- an rx / tx batch's submit may still be running --
    // is first waited for: finished (its batch's poll then sees it done), or
    // withdrawn unrun (the poll sees that and launches it).  Only then may
    // another thread claim the slot and post on it: a job number the slot's
    // next holder reuses can no longer be mistaken for this thread's.  False:
    // the job neither finished nor left in time -- the slot stays taken.
    bool release(int b, uint64_t me)
    {
        if (b < 0 || b >= kResSlots || !mb_) return true;
        if (__atomic_load_n(&hs_[b].owner, __ATOMIC_ACQUIRE) != me) return true;  // not this thread's
        const uint64_t s = hs_[b].seq;
        if (s && hs_[b].cancelled != s && !all_done(mb_->slot[b], s, hs_[b].parts)) {
            n_.add(Counters::kDrained);
            if (wait(b, s) == KMWS_ERR_TIMEOUT) return false;
        }
        __atomic_store_n(&hs_[b].owner, 0ull, __ATOMIC_RELEASE);
        if (!__atomic_load_n(&exiting_, __ATOMIC_ACQUIRE))
            __atomic_fetch_and(&mb_->slot[b].word, ~kClaimedBit, __ATOMIC_RELEASE);
        __atomic_fetch_and(&claimed_, ~(1u << b), __ATOMIC_ACQ_REL);
        return true;
    }
    // A thread whose slots were given back at its exit asked for a job: it
    // launches instead (counted).
    void note_late_post() { n_.add(Counters::kLatePosts); }

    // Ask every workgroup to leave at its next poll and wait for the grid (atexit).
    void quit_and_wait()
    {
        __atomic_store_n(&exiting_, true, __ATOMIC_RELEASE);
        if (!mb_) return;
        std::lock_guard<std::mutex> lk(launch_mu_);
        state_ = -1;  // no relaunch from here on
        for (int b = 0; b < kResSlots; ++b) __atomic_fetch_or(&mb_->slot[b].word, kQuitBit, __ATOMIC_RELEASE);
        const uint64_t cur = ld_acq(&inc_);
        const auto t0 = Clock::now();
        while (cur && ld_acq(&mb_->exited) != cur && Clock::now() - t0 < std::chrono::milliseconds(500)) cpu_relax();
    }

    // created on first use: a process whose threads all switched the worker
    // off creates nothing (no stream, no mailbox)
    bool usable()
    {
        int s = ld_acq(&state_);
        if (s == 0) {
            std::lock_guard<std::mutex> lk(launch_mu_);
            if (state_ == 0) state_ = init() == KMWS_OK ? 1 : -1;
            s = state_;
        }
        return s == 1;
    }

    // Posts one job of n <= kResMaxDescs payloads on slot b (held by the
    // calling thread) and returns without waiting; *job = its number.
    // KMWS_ERR_NOT_SUPPORTED: the slot's previous job is still running, or the
    // worker cannot be (re)launched -- nothing was posted.
    // ck: a checked job (its views, verdict bytes and the payloads' host
    // addresses), which only the validating instantiation takes: from the first
    // one on every incarnation of this worker is launched as that one, and an
    // unchecked incarnation it meets is asked to leave (KMWS_ERR_NOT_SUPPORTED:
    // this caller launches).
    kmws_status post(int b, uint64_t me, const ResDesc* d, uint32_t n, uint64_t* job, const ResCheckArgs* ck = nullptr)
    {
        if (n == 0 || n > (uint32_t)kResMaxDescs || !usable()) return KMWS_ERR_NOT_SUPPORTED;
        for (uint32_t i = 0; i < n; ++i)
            if ((d[i].addr & ~kAddrMask) != 0 || d[i].len > kLenMask) return KMWS_ERR_NOT_SUPPORTED;
        if (ck && (ck->verdict & ~kAddrMask) != 0) return KMWS_ERR_NOT_SUPPORTED;
        if (ck && !ld_acq(&checked_seen_)) __atomic_store_n(&checked_seen_, true, __ATOMIC_RELEASE);
        // only the slot's holder writes its descriptors and job word: a post
        // from any other thread is refused (and counted -- never expected)
        if (__atomic_load_n(&hs_[b].owner, __ATOMIC_ACQUIRE) != me) {
            n_.add(Counters::kUnownedPosts);
            return KMWS_ERR_NOT_SUPPORTED;
        }
        ResSlot& sl = mb_->slot[b];
        const uint64_t prev = hs_[b].seq;
        uint64_t cur = ld_acq(&inc_);
        if (hs_[b].cancelled != prev && !all_done(sl, prev, hs_[b].parts)) {  // busy: the caller launches
            // (a job a previous holder left posted: a grid that left is relaunched for it)
            if (cur && ld_acq(&mb_->exited) == cur) (void)relaunch(cur);
            return KMWS_ERR_NOT_SUPPORTED;
        }
        if (cur == 0 || ld_acq(&mb_->exited) == cur) cur = relaunch(cur);
        if (cur == 0) return KMWS_ERR_NOT_SUPPORTED;
        // a slot claimed after the running incarnation was launched has no
        // workgroups in it: that incarnation was asked to leave (claim); launch
        // until it has, and the next post relaunches
        if ((uint32_t)b >= ld_acq(&nslots_)) {
            request_resize(cur);
            return KMWS_ERR_NOT_SUPPORTED;
        }
        // the incarnation serving is the unchecked instantiation: it leaves as
        // for a resize, and the relaunch (the next post) is the validating one
        if (ck && !ld_acq(&inc_checked_)) {
            if (__atomic_exchange_n(&switch_inc_, cur, __ATOMIC_ACQ_REL) != cur) n_.add(Counters::kVariantSwitches);
            request_resize(cur);
            return KMWS_ERR_NOT_SUPPORTED;
        }
        const uint64_t s = (prev + 1) & kJobMask;
        uint64_t words = 0;
        for (uint32_t i = 0; i < n; ++i) words += hull_words(d[i].addr, d[i].len);
        const uint32_t parts = part_count(words);
        if (ck && !checked_fits(words, parts)) return KMWS_ERR_NOT_SUPPORTED;
        if (ck) {
            for (uint32_t i = 0; i < n; ++i) __atomic_store_n(&sl.view[i], ck->view[i], __ATOMIC_RELAXED);
            // the dword before each later part's first word, read before any
            // workgroup can have stored it (edge_pick: the device's own split)
            for (uint32_t p = 1; p < parts; ++p) {
                const EdgePick e = edge_pick(d, n, (uint32_t)words, p, parts);
                uint32_t edge = 0;
                if (e.index >= 0) {
                    const uintptr_t first = reinterpret_cast<uintptr_t>(ck->host[e.index]) & ~(uintptr_t)15;
                    std::memcpy(&edge, reinterpret_cast<const uint8_t*>(first + e.offset), 4);
                }
                __atomic_store_n(&sl.edge[p], (uint64_t)edge, __ATOMIC_RELAXED);
            }
        }
        // (tagged like a descriptor; once a checked job was seen every job
        // rewrites it, so a stale one always carries job s - 1's tag)
        if (ck || ld_acq(&checked_seen_))
            __atomic_store_n(&sl.verdict, tag_verdict(ck ? ck->verdict : 0ull, s), __ATOMIC_RELAXED);
        const bool wt = words <= (uint64_t)kResWriteThroughWords || device_batch_running(device_);
        n_.add(wt ? Counters::kWtJobs : Counters::kReleasedJobs);
        // every polled slot is rewritten, so a stale half always carries job s - 1's tag
        for (uint32_t i = 0; i < n || i < (uint32_t)kPollDescs; ++i) {
            const ResDesc x = tag_desc(i < n ? d[i] : ResDesc{0, 0, 0}, s);
            uint64_t* q = reinterpret_cast<uint64_t*>(&sl.desc[i]);
            __atomic_store_n(q, x.addr, __ATOMIC_RELAXED);
            __atomic_store_n(q + 1, (uint64_t)x.len | (uint64_t)x.key << 32, __ATOMIC_RELAXED);
        }
        __atomic_store_n(&hs_[b].parts, parts, __ATOMIC_RELAXED);
        __atomic_store_n(&hs_[b].seq, s, __ATOMIC_RELEASE);
        __atomic_store_n(&hs_[b].jobs, hs_[b].jobs + 1, __ATOMIC_RELAXED);  // (a withdrawn job is taken off again)
        __atomic_store_n(&hs_[b].checked, ck != nullptr, __ATOMIC_RELAXED);
        if (ck) __atomic_store_n(&hs_[b].checked_jobs, hs_[b].checked_jobs + 1, __ATOMIC_RELAXED);
        const uint64_t flags = (wt ? kWriteThroughBit : 0) | (ck ? kCheckBit : 0) | kClaimedBit;
        __atomic_store_n(&sl.word, pack_job(s, n, parts, flags), __ATOMIC_RELEASE);
        *job = s;
        return KMWS_OK;
    }

    // 1 when job s of slot b is done, 0 while it runs (relaunching a grid that
    // left before taking it), KMWS_ERR_NOT_SUPPORTED when it was withdrawn
    // (never run: the caller launches it).
    int test(int b, uint64_t s)
    {
        if (withdrawn_job(b, s)) return KMWS_ERR_NOT_SUPPORTED;
        if (finished(b, s)) return 1;
        const uint64_t cur = ld_acq(&inc_);
        if (ld_acq(&mb_->exited) == cur) {
            if (finished(b, s)) return 1;
            if (relaunch(cur) == 0 && withdraw(b, s, cur)) return KMWS_ERR_NOT_SUPPORTED;
        }
        return 0;
    }

    // Waits for job s of slot b.  KMWS_OK: done.  KMWS_ERR_NOT_SUPPORTED:
    // withdrawn without having run (payloads untouched; the caller launches).
    // KMWS_ERR_TIMEOUT: the workgroup holding it neither finished nor left
    // within the bounds -- the device may still write its payloads.
    kmws_status wait(int b, uint64_t s)
    {
        ResSlot& sl = mb_->slot[b];
        if (withdrawn_job(b, s)) return KMWS_ERR_NOT_SUPPORTED;  // (by its thread's release at exit)
        const auto t0 = Clock::now();
        Clock::time_point orphan{};
        for (uint32_t spin = 0;; ++spin) {
            if (finished(b, s)) return KMWS_OK;
            cpu_relax();
            if ((spin & 255) != 255) continue;
            const uint64_t cur = ld_acq(&inc_);
            if (ld_acq(&mb_->exited) == cur) {  // the whole grid left: relaunch (the new one takes job s)
                if (finished(b, s)) return KMWS_OK;
                if (relaunch(cur) == 0) {
                    if (withdraw(b, s, cur)) return KMWS_ERR_NOT_SUPPORTED;
                    continue;
                }
                orphan = Clock::time_point{};
            } else if (part_left(sl, s, hs_[b].parts, cur)) {  // a part's workgroup left, others run on
                if (finished(b, s)) return KMWS_OK;
                const auto now = Clock::now();
                if (orphan == Clock::time_point{}) orphan = now;
                else if (now - orphan > std::chrono::microseconds(kResOrphanUs) && withdraw(b, s, cur))
                    return KMWS_ERR_NOT_SUPPORTED;
            } else {
                orphan = Clock::time_point{};
            }
            if (Clock::now() - t0 > std::chrono::milliseconds(KMWS_RESIDENT_TIMEOUT_MS)) return timed_out(b, s);
        }
    }

    uint64_t jobs(bool checked = false) const  // jobs (checked ones) posted and not withdrawn, over the slots
    {
        uint64_t n = 0;
        for (const SlotHost& h : hs_) n += __atomic_load_n(checked ? &h.checked_jobs : &h.jobs, __ATOMIC_RELAXED);
        return n;
    }
    uint64_t count(Counters::Id i) const { return n_.get(i); }
    uint64_t launches() const { return ld_acq(&inc_); }
    int claimed() const { return __builtin_popcount(ld_acq(&claimed_)); }
    // Workgroup exits so far by reason (ResCtl::why), read from device memory.
    kmws_status exit_reasons(uint64_t* out, int n)
    {
        if (!dctl_) {
            for (int i = 0; i < n; ++i) out[i] = 0;
            return KMWS_OK;
        }
        uint64_t w[kResExitReasons] = {};
        DevGuard g(device_);
        if (hipMemcpy(w, dctl_->why, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return KMWS_ERR_FAILED;
        }
        for (int i = 0; i < n; ++i) out[i] = i < kResExitReasons ? w[i] : 0;
        return KMWS_OK;
    }
    int running() const
    {
        const uint64_t cur = ld_acq(&inc_);
        return mb_ && cur && ld_acq(&mb_->exited) != cur ? 1 : 0;
    }

private:
    // Every part of job s finished?  (A part's done word at or past s.)
    static bool all_done(const ResSlot& sl, uint64_t s, uint32_t parts)
    {
        for (uint32_t j = 0; j < parts; ++j)
            if (!job_done(ld_acq(&sl.done[j]), s)) return false;
        return true;
    }
    // Job s of slot b finished -- or the slot has moved on (a later job is
    // posted only once s was finished or withdrawn, by s's own waiter).
    // (Read by the job's poller, which after a release at thread exit may not
    // be the slot's holder any more: atomic loads.)
    bool finished(int b, uint64_t s) const
    {
        return ld_acq(&hs_[b].seq) != s || all_done(mb_->slot[b], s, ld_acq(&hs_[b].parts));
    }
    // Job s of slot b was withdrawn unrun (by its waiter, or by the release at
    // its thread's exit): its caller launches it.
    bool withdrawn_job(int b, uint64_t s) const { return ld_acq(&hs_[b].cancelled) == s; }
    // Part j of job s, seen from grid `cur` (all_left: its last workgroup has exited).
    static Part part_state(const ResSlot& sl, uint32_t j, uint64_t s, uint64_t cur, bool all_left)
    {
        if (job_done(ld_acq(&sl.done[j]), s)) return Part::kFinished;
        return all_left || ld_acq(&sl.gone[j]) == cur ? Part::kLeft : Part::kHeld;
    }
    // Has the workgroup of an unfinished part of job s left grid `cur` (which still runs)?
    static bool part_left(const ResSlot& sl, uint64_t s, uint32_t parts, uint64_t cur)
    {
        for (uint32_t j = 0; j < parts; ++j)
            if (part_state(sl, j, s, cur, false) == Part::kLeft) return true;
        return false;
    }

    // Takes job s of slot b back if no workgroup ran any of it and none can
    // take it any more: the grid `cur` is still the latest (no relaunch can
    // start while launch_mu_ is held) and the workgroup of every part has left.
    // The word keeps the job number with the cancel bit (and the quit bit
    // cleared), so no workgroup -- of this grid or a later one -- runs it; the
    // slot's next job takes the next number.  False: a part ran (or runs), or
    // a newer grid will take it.
    bool withdraw(int b, uint64_t s, uint64_t cur)
    {
        ResSlot& sl = mb_->slot[b];
        std::lock_guard<std::mutex> lk(launch_mu_);
        if (ld_acq(&inc_) != cur || hs_[b].seq != s) return false;
        const bool all_left = ld_acq(&mb_->exited) == cur;
        for (uint32_t j = 0; j < hs_[b].parts; ++j)
            if (part_state(sl, j, s, cur, all_left) != Part::kLeft) return false;
        __atomic_store_n(&sl.word, (ld_acq(&sl.word) | kCancelBit) & ~kQuitBit, __ATOMIC_RELEASE);
        __atomic_store_n(&hs_[b].cancelled, s, __ATOMIC_RELEASE);
        n_.add(Counters::kWithdrawn);
        __atomic_store_n(&hs_[b].jobs, hs_[b].jobs - 1, __ATOMIC_RELAXED);
        if (__atomic_load_n(&hs_[b].checked, __ATOMIC_RELAXED)) __atomic_store_n(&hs_[b].checked_jobs, hs_[b].checked_jobs - 1, __ATOMIC_RELAXED);
        return true;
    }

    // Past the timeout: the quit bit asks slot b's workgroup to leave (it may
    // be inside the job, or stuck); wait, bounded, until it has.
    kmws_status timed_out(int b, uint64_t s)
    {
        ResSlot& sl = mb_->slot[b];
        const uint32_t parts = hs_[b].parts;
        n_.add(Counters::kTimeouts);
        __atomic_fetch_or(&sl.word, kQuitBit, __ATOMIC_RELEASE);
        const auto t0 = Clock::now();
        for (uint32_t spin = 0;; ++spin) {
            if (finished(b, s)) {
                std::lock_guard<std::mutex> lk(launch_mu_);
                __atomic_fetch_and(&sl.word, ~kQuitBit, __ATOMIC_RELEASE);
                return KMWS_OK;
            }
            cpu_relax();
            if ((spin & 255) != 255) continue;
            const uint64_t cur = ld_acq(&inc_);
            const bool all_left = ld_acq(&mb_->exited) == cur;
            bool settled = true;  // every part finished, or its workgroup left
            for (uint32_t j = 0; j < parts; ++j) settled &= part_state(sl, j, s, cur, all_left) != Part::kHeld;
            if (settled) {
                if (withdraw(b, s, cur)) return KMWS_ERR_NOT_SUPPORTED;  // no part ran: the caller launches
                // some parts ran: the others run in the next grid (the quit bit cleared)
                {
                    std::lock_guard<std::mutex> lk(launch_mu_);
                    __atomic_fetch_and(&sl.word, ~kQuitBit, __ATOMIC_RELEASE);
                }
                if (all_left) (void)relaunch(cur);
            }
            if (Clock::now() - t0 > std::chrono::milliseconds(KMWS_RESIDENT_DRAIN_MS)) break;
        }
        // still held by a workgroup that does not leave: the payloads stay the
        // device's, and no job is posted on this device's worker again
        std::lock_guard<std::mutex> lk(launch_mu_);
        state_ = -1;
        return KMWS_ERR_TIMEOUT;
    }

    kmws_status init()  // under launch_mu_
    {
        if (device_ < 0 || kmws_device_count() <= device_) return KMWS_ERR_NOT_SUPPORTED;
        DevGuard g(device_);
        void* p = nullptr;
        if (hipHostMalloc(&p, sizeof(ResMailbox), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            return KMWS_ERR_FAILED;
        }
        mb_ = static_cast<ResMailbox*>(p);
        std::memset(static_cast<void*>(mb_), 0, sizeof(ResMailbox));
        dmb_ = static_cast<ResMailbox*>(device_view(mb_));
        if (!dmb_) return KMWS_ERR_FAILED;
        // uncached: every XCD's workgroups read and update these words
        if (hipExtMallocWithFlags(reinterpret_cast<void**>(&dctl_), sizeof(ResCtl), hipDeviceMallocUncached) !=
            hipSuccess) {
            (void)hipGetLastError();
            dctl_ = nullptr;
            if (hipMalloc(reinterpret_cast<void**>(&dctl_), sizeof(ResCtl)) != hipSuccess) {
                (void)hipGetLastError();
                return KMWS_ERR_FAILED;
            }
        }
        // A non-blocking stream: the legacy default stream (torch's current stream
        // unless the caller picked another) waits for every blocking stream's
        // work, which would include this kernel -- measured: a kernel on the null
        // stream behind a CU-masked (blocking) worker stream waited out its idle
        // time, 5.02 ms each time.  At the greatest priority: the runtime keeps
        // separate hardware queues per priority, so the worker does not share a
        // queue with the process's ordinary streams unless those ask for the
        // same priority (the lease bounds the wait when they do).
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) {
            (void)hipGetLastError();
            greatest = least = 0;
        }
        // The grid runs on the SECOND greatest-priority stream this worker makes:
        // on the first one, a device batch beside the grid ran 1.33-1.40x slower
        // (cfg2, 0.82 -> 0.59 of HBM peak) whatever the grid did -- its jobs, its
        // polls, its block size, its lease (every such variant measured, and a
        // probe kernel of the grid's shape on a stream of its own slowed nothing);
        // with a greatest-priority stream made before it the same grid cost
        // 1.02x under 16 threads' 4 KiB masks (tools/grid_interference.cpp,
        // tools/priority_probe.hip, profiles/r06ag_*).  The spare stays unused.
        if (hipStreamCreateWithPriority(&spare_stream_, hipStreamNonBlocking, greatest) != hipSuccess ||
            hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();
            return KMWS_ERR_FAILED;
        }
        // cleared on the worker's own stream: a device-wide synchronize here
        // would wait for every stream of the process (a long kernel elsewhere),
        // with launch_mu_ held
        if (hipMemsetAsync(dctl_, 0, sizeof(ResCtl), stream_) != hipSuccess ||
            hipStreamSynchronize(stream_) != hipSuccess) {
            (void)hipGetLastError();
            return KMWS_ERR_FAILED;
        }
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_) != hipSuccess || khz <= 0)
            khz = 100000;  // gfx9 constant clock: 100 MHz
        idle_ticks_ = (uint64_t)khz * kResIdleUs / 1000u;
        lease_ticks_ = (uint64_t)khz * kResLeaseUs / 1000u;
        // registered after the HIP runtime initialised (the calls above), so at
        // exit it runs before the runtime's own teardown
        static std::once_flag once;
        std::call_once(once, [] { std::atexit(quit_all_workers); });
        return KMWS_OK;
    }

    // Incarnations up to `cur` leave at their next few polls (monotonic).
    void request_resize(uint64_t cur)
    {
        uint64_t r = ld_acq(&mb_->resize);
        while (r < cur && !__atomic_compare_exchange_n(&mb_->resize, &r, cur, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
        }
    }

    // Launches the next incarnation once `seen` (0: none yet) has left
    // entirely; returns the incarnation now serving, or 0 if the worker is
    // unusable (nothing launched).
    uint64_t relaunch(uint64_t seen)
    {
        std::lock_guard<std::mutex> lk(launch_mu_);
        if (state_ != 1) return 0;
        const uint64_t cur = inc_;
        if (cur != seen) return cur;                                   // another thread relaunched
        if (cur != 0 && ld_acq(&mb_->exited) != cur) return cur;      // still running
        // the slots claimed now, up to the highest (a slot claimed later is
        // served from the next incarnation on; its jobs launch until then)
        const uint32_t m = ld_acq(&claimed_);
        const uint32_t nslots = m ? 32u - (uint32_t)__builtin_clz(m) : 1u;
        DevGuard g(device_);
        // the instantiation is chosen per incarnation: the validating one from
        // the first checked job posted on this device on, never before
        const bool chk = ld_acq(&checked_seen_);
        hipLaunchKernelGGL(chk ? resident_unmask_kernel<true> : resident_unmask_kernel<false>, dim3(nslots * kResParts),
                           dim3(kResBlock), 0, stream_, dmb_, dctl_, cur + 1, nslots, exit_base_, idle_ticks_, lease_ticks_);
        if (hipGetLastError() != hipSuccess) {
            state_ = -1;
            return 0;
        }
        __atomic_store_n(&inc_checked_, chk, __ATOMIC_RELEASE);
        exit_base_ += (uint64_t)nslots * kResParts;
        __atomic_store_n(&nslots_, nslots, __ATOMIC_RELEASE);
        __atomic_store_n(&inc_, cur + 1, __ATOMIC_RELEASE);
        return cur + 1;
    }

    int device_;
    std::mutex launch_mu_;
    int state_ = 0;  // 0 untried, 1 ready, -1 unusable
    bool exiting_ = false;
    uint32_t claimed_ = 0;  // bit b: slot b held by a thread
    ResMailbox* mb_ = nullptr;
    ResMailbox* dmb_ = nullptr;
    ResCtl* dctl_ = nullptr;
    hipStream_t stream_ = nullptr;
    hipStream_t spare_stream_ = nullptr;  // made first, never used (see init)
    uint64_t idle_ticks_ = 0, lease_ticks_ = 0;
    uint64_t inc_ = 0;  // latest incarnation launched
    uint32_t nslots_ = 0;     // slots the latest incarnation serves
    uint64_t exit_base_ = 0;  // workgroups launched in all incarnations so far
    // Per slot, written by its holder thread (a withdraw by the holder too,
    // under launch_mu_), each on a cache line of its own: a thread spinning on
    // its job reads its own line only, and another thread's post does not
    // invalidate it (16 threads shared three arrays and one job counter before).
    struct alignas(64) SlotHost {
        uint64_t seq = 0;        // last job number posted
        uint64_t cancelled = 0;  // the last job withdrawn
        uint64_t jobs = 0;       // jobs posted and not withdrawn (summed by jobs())
        uint64_t owner = 0;      // owner token of the thread holding the slot (0: free)
        uint32_t parts = 0;      // parts of job `seq`
        bool checked = false;    // job `seq` is a checked one
        uint64_t checked_jobs = 0;  // checked jobs posted and not withdrawn
    };
    SlotHost hs_[kResSlots];
    alignas(64) Counters n_;  // off the slots' lines
    bool checked_seen_ = false;   // a checked job was posted: incarnations are the validating one from now on
    bool inc_checked_ = false;    // the latest incarnation is the validating one
    uint64_t switch_inc_ = 0;     // the last incarnation asked to leave for it
};

// Every worker of the process (for the exit handler); never freed.
std::mutex g_all_mu;
std::vector<ResidentWorker*>* g_all = nullptr;

void quit_all_workers()
{
    std::lock_guard<std::mutex> lk(g_all_mu);
    if (g_all)
        for (ResidentWorker* w : *g_all) w->quit_and_wait();
}

constexpr int kMaxDevices = 64;
ResidentWorker* g_by_dev[kMaxDevices];  // set once under g_all_mu, read with acquire loads

ResidentWorker* worker(int device)
{
    if (device < 0 || device >= kMaxDevices) return nullptr;
    ResidentWorker* w = __atomic_load_n(&g_by_dev[device], __ATOMIC_ACQUIRE);
    if (w) return w;
    std::lock_guard<std::mutex> lk(g_all_mu);
    w = g_by_dev[device];
    if (!w) {
        w = new (std::nothrow) ResidentWorker(device);
        if (!w) return nullptr;
        if (!g_all) g_all = new std::vector<ResidentWorker*>();
        g_all->push_back(w);
        __atomic_store_n(&g_by_dev[device], w, __ATOMIC_RELEASE);
    }
    return w;
}

// The calling thread's slots, one per device.  Plain data -- zero-initialised,
// trivially destructible -- so it stays valid while the thread's other
// thread_local objects are destroyed, before and after ThreadExit below gives
// the slots back.  slot1[d] = slot + 1 (0: none held; -1: its job timed out,
// the slot is never given back).  kmws_resident_enable(0) makes the thread's
// calls launch instead (the A/B of the worker) and gives its slot back.
struct ThreadSlots {
    int8_t slot1[kMaxDevices];
    uint64_t off_mask;  // bit d: worker off for device d on this thread
    uint64_t token;     // this thread's owner token (0 until its first claim)
    bool gone;          // its slots were given back at thread exit: later jobs launch
};
thread_local ThreadSlots t_slots;

// The calling thread gives its slot on `device` back, if it holds one (kept,
// as -1, where its last job neither finished nor left in time).
void give_back(int device)
{
    if (t_slots.slot1[device] <= 0) return;
    ResidentWorker* w = __atomic_load_n(&g_by_dev[device], __ATOMIC_ACQUIRE);
    t_slots.slot1[device] = !w || w->release(t_slots.slot1[device] - 1, t_slots.token) ? 0 : -1;
}

// Gives the thread's slots back when it exits.  Constructed at the thread's
// first claim (or by kmws_thread_attach), so C++'s reverse order of
// thread_local destruction runs it after every thread_local object that was
// complete by then -- and before those completed later.  VERDICT r05: a
// thread_local RxLoop / TxLoop made before the thread's first job was
// destroyed AFTER the slot had been given back, and its flush posted on a slot
// another thread might hold by then (both wrote the same job number).  Now
// such a flush finds `gone` set and launches; a loop that attached in its
// constructor is destroyed first and flushes on its slot.
struct ThreadExit {
    bool armed = false;
    ~ThreadExit()
    {
        t_slots.gone = true;
        for (int d = 0; d < kMaxDevices; ++d) give_back(d);
    }
};
thread_local ThreadExit t_exit;

uint64_t g_next_token = 0;

// The calling thread's slot on `device` (claimed on first use), or -1.
int thread_slot(int device, ResidentWorker** wout)
{
    if (device < 0 || device >= kMaxDevices || ((t_slots.off_mask >> device) & 1u)) return -1;
    ResidentWorker* w = worker(device);
    if (!w) return -1;
    *wout = w;
    if (t_slots.gone) {  // past this thread's ThreadExit: nothing is claimed any more
        w->note_late_post();
        return -1;
    }
    const int s1 = t_slots.slot1[device];
    if (s1 != 0) return s1 - 1;  // held (or -2: kept by a timed-out job)
    if (!t_slots.token) t_slots.token = __atomic_add_fetch(&g_next_token, 1, __ATOMIC_RELAXED);
    t_exit.armed = true;  // constructs it before the claim: the slot is given back at exit
    const int b = w->claim(t_slots.token);
    if (b >= 0) t_slots.slot1[device] = (int8_t)(b + 1);
    return b;
}

}  // namespace

// Posts the unmask of descs[0..n) over dev_base and descs2[0..n2) over
// dev_base2 (device views of pinned host memory, offsets relative to them) on
// the calling thread's slot; see kmws_common.hpp.
kmws_status resident_post(int device, const kmws_desc* descs, const uint8_t* dev_base, size_t n,
                          const kmws_desc* descs2, const uint8_t* dev_base2, size_t n2, ResidentJob* job,
                          uint64_t max_bytes, const ResidentCheck* check)
{
    if (n + n2 == 0 || n + n2 > (size_t)kResMaxDescs) return KMWS_ERR_NOT_SUPPORTED;
    if (check && (!check->verdict_dv || (n && !check->host_base) || (n2 && !check->host_base2)))
        return KMWS_ERR_INVALID_PARAM;
    ResidentWorker* w = nullptr;
    const int b = thread_slot(device, &w);
    if (b < 0) return KMWS_ERR_NOT_SUPPORTED;
    ResDesc d[kResMaxDescs];
    ResCheckArgs ck;
    // a view that is not checked, or whose verdict byte does not exist: only unmasked
    auto view_word = [&](const Utf8View* v) -> uint64_t {
        if (!v || !(v->w & kUtf8Checked) || v->slot >= check->n_verdict) return 0ull;
        return (uint64_t)(v->w & (0xFFFFFFu | kUtf8Checked)) | (uint64_t)v->slot << 32;
    };
    uint64_t bytes = 0;
    size_t k = 0;
    // one source: its descriptors over `dev`, the first n_views of them with a view, host addresses over `host`
    auto add = [&](const kmws_desc* src, size_t cnt, const uint8_t* dev, const Utf8View* views, size_t n_views,
                   const uint8_t* host) {
        for (size_t i = 0; i < cnt; ++i, ++k) {
            d[k] = ResDesc{(uint64_t)(uintptr_t)(dev + src[i].off), src[i].len, src[i].key};
            bytes += src[i].len;
            if (check) {
                ck.view[k] = view_word(views && i < n_views ? &views[i] : nullptr);
                ck.host[k] = host + src[i].off;
            }
        }
    };
    add(descs, n, dev_base, check ? check->views : nullptr, n, check ? check->host_base : nullptr);
    add(descs2, n2, dev_base2, check ? check->views2 : nullptr, check ? check->n_views2 : 0,
        check ? check->host_base2 : nullptr);
    if (bytes > max_bytes || bytes > kResMaxBytes) return KMWS_ERR_NOT_SUPPORTED;
    if (check) ck.verdict = (uint64_t)(uintptr_t)check->verdict_dv;
    uint64_t s = 0;
    const kmws_status st = w->post(b, t_slots.token, d, (uint32_t)k, &s, check ? &ck : nullptr);
    if (st != KMWS_OK) return st;
    job->device = device;
    job->slot = b;
    job->seq = s;
    return KMWS_OK;
}

int resident_test(const ResidentJob& job)
{
    ResidentWorker* w = worker(job.device);
    return w ? w->test(job.slot, job.seq) : KMWS_ERR_INVALID_PARAM;
}

kmws_status resident_wait(const ResidentJob& job)
{
    ResidentWorker* w = worker(job.device);
    if (!w) return KMWS_ERR_INVALID_PARAM;
    const kmws_status st = w->wait(job.slot, job.seq);
    if (st == KMWS_ERR_TIMEOUT && job.device >= 0 && job.device < kMaxDevices &&
        t_slots.slot1[job.device] == job.slot + 1)
        t_slots.slot1[job.device] = -1;  // the slot stays the device's
    return st;
}

kmws_status resident_unmask(int device, const kmws_desc* descs, const uint8_t* dev_base, size_t n,
                            const kmws_desc* descs2, const uint8_t* dev_base2, size_t n2)
{
    ResidentJob job;
    const kmws_status st = resident_post(device, descs, dev_base, n, descs2, dev_base2, n2, &job);
    return st != KMWS_OK ? st : resident_wait(job);
}

}  // namespace kmws

extern "C" {

kmws_status kmws_resident_enable(int device, int on)
{
    if (device < 0 || device >= kmws::kMaxDevices) return KMWS_ERR_INVALID_PARAM;
    kmws::ThreadSlots& ts = kmws::t_slots;
    if (on) {
        ts.off_mask &= ~(1ull << device);
    } else {
        ts.off_mask |= 1ull << device;
        kmws::give_back(device);
    }
    return KMWS_OK;
}

kmws_status kmws_resident_info(int device, uint64_t* jobs, uint64_t* launches, int* running)
{
    kmws::ResidentWorker* w = kmws::worker(device);
    if (!w) return KMWS_ERR_INVALID_PARAM;
    if (jobs) *jobs = w->jobs();
    if (launches) *launches = w->launches();
    if (running) *running = w->running();
    return KMWS_OK;
}

kmws_status kmws_resident_counters(int device, int* thread_slot, int* slots_claimed, uint64_t* timeouts,
                                   uint64_t* withdrawn)
{
    kmws::ResidentWorker* w = kmws::worker(device);
    if (!w) return KMWS_ERR_INVALID_PARAM;
    if (thread_slot) *thread_slot = kmws::t_slots.slot1[device] > 0 ? kmws::t_slots.slot1[device] - 1 : -1;
    if (slots_claimed) *slots_claimed = w->claimed();
    if (timeouts) *timeouts = w->count(kmws::Counters::kTimeouts);
    if (withdrawn) *withdrawn = w->count(kmws::Counters::kWithdrawn);
    return KMWS_OK;
}

kmws_status kmws_resident_guard_counters(int device, uint64_t* unowned_posts, uint64_t* late_posts,
                                         uint64_t* drained_releases)
{
    kmws::ResidentWorker* w = kmws::worker(device);
    if (!w) return KMWS_ERR_INVALID_PARAM;
    if (unowned_posts) *unowned_posts = w->count(kmws::Counters::kUnownedPosts);
    if (late_posts) *late_posts = w->count(kmws::Counters::kLatePosts);
    if (drained_releases) *drained_releases = w->count(kmws::Counters::kDrained);
    return KMWS_OK;
}

kmws_status kmws_resident_store_counters(int device, uint64_t* write_through, uint64_t* released)
{
    kmws::ResidentWorker* w = kmws::worker(device);
    if (!w) return KMWS_ERR_INVALID_PARAM;
    if (write_through) *write_through = w->count(kmws::Counters::kWtJobs);
    if (released) *released = w->count(kmws::Counters::kReleasedJobs);
    return KMWS_OK;
}

kmws_status kmws_resident_utf8_counters(int device, uint64_t* checked_jobs, uint64_t* variant_switches)
{
    if (device < 0 || device >= kmws::kMaxDevices || kmws_device_count() <= device) return KMWS_ERR_INVALID_PARAM;
    kmws::ResidentWorker* w = kmws::worker(device);
    if (!w) return KMWS_ERR_INVALID_PARAM;
    if (checked_jobs) *checked_jobs = w->jobs(true);
    if (variant_switches) *variant_switches = w->count(kmws::Counters::kVariantSwitches);
    return KMWS_OK;
}

int kmws_device_batch_busy(int device) { return kmws::device_batch_running(device) ? 1 : 0; }

int kmws_thread_attach(int device)
{
    if (device == KMWS_DEVICE_AUTO) device = kmws_thread_device();
    if (device < 0 || device >= kmws::kMaxDevices || kmws_device_count() <= device) return KMWS_ERR_NOT_SUPPORTED;
    kmws::ResidentWorker* w = nullptr;
    const int b = kmws::thread_slot(device, &w);
    // even without a slot (all taken, worker off): the thread's exit hook now
    // exists, so a slot claimed later is still given back after this caller's
    // thread_local objects
    if (!kmws::t_slots.gone) kmws::t_exit.armed = true;
    return b;
}

kmws_status kmws_resident_exit_reasons(int device, uint64_t* counts, int n)
{
    kmws::ResidentWorker* w = kmws::worker(device);
    if (!w || !counts || n < 0) return KMWS_ERR_INVALID_PARAM;
    return w->exit_reasons(counts, n);
}

}  // extern "C"
