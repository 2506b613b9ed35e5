// The resident worker's mailbox format (kmws_resident.hip), in one place: the job word's bits, the descriptor
// and verdict tags, the split of a job's hull words over its parts, the slots' layout.  Plain structs and
// __host__ __device__ inline code only -- no HIP runtime call, no atomic, no load from the mailbox -- so the
// host checks it as a program (tests/cpp/resident_proto_check.cpp).
#pragma once
#include <stddef.h>

#include "kmws_common.hpp"

namespace kmws {

constexpr int kResBlock = 1024;  // 16 waves: 4 words each = 64 KiB of loads in flight
constexpr int kResWords = 4;
// Slots per device: one per loop thread that uses the synchronous entries
// (kuma's test client runs 10 loop threads, its server 5).  Unclaimed slots'
// workgroups poll one word every few microseconds; a claimed slot's workgroup
// polls its job word and 31 descriptor slots (512 B) back to back.
constexpr int kResSlots = 16;
// Workgroups per slot: one CU moves ~13 GB/s of a job's PCIe traffic (the misses
// it keeps in flight to host memory bound it, not its lanes), so a job of at
// least 2 x kPartWords words is split over up to kResParts workgroups, each
// polling the slot's job word itself.
constexpr int kResParts = 4;
constexpr uint32_t kPartWords = 1024;  // 16 KiB: the least a part takes

struct ResDesc {  // one payload: device-visible address, bytes, LE key of its first byte
    uint64_t addr;
    uint32_t len;
    uint32_t key;
};
static_assert(sizeof(ResDesc) == 16, "ResDesc is one 16-byte load");

// The polled word of a slot: job number (bits 0-39), payload count (40-47),
// parts - 1 (48-49: the workgroups the job is split over), cancelled (61: a
// job its thread withdrew -- no workgroup runs it), claimed (62: a thread holds
// the slot, so its part-0 workgroup polls the descriptors too) and quit (63).
// The first kPollDescs descriptor slots follow it and are read with it at
// every poll of part 0, so a job of up to kPollDescs payloads costs one PCIe
// round trip to notice and none more to read its descriptors.  The host
// rewrites every one of those slots for every job (unused ones with length 0),
// each as two 8-byte stores tagged with the job's low bits (address bits
// 48-63; length bits 21-31 in the half that also holds the key): a half read
// before the host's write landed carries the previous job's tag, and the job's
// descriptors are then read again after the word.
constexpr uint64_t kJobMask = (1ull << 40) - 1;
constexpr int kCountShift = 40;
constexpr int kPartShift = 48;
constexpr uint64_t kWriteThroughBit = 1ull << 50;  // the job's stores write through (no release)
// A checked job (kmws_decoder_set_utf8_check): its text payloads are validated
// in the pass that unmasks them.  Only the validating instantiation of the
// kernel takes one (ResidentWorker::post); the slot's view words, edge words
// and the verdict word beside the job word belong to it (ResSlot).
constexpr uint64_t kCheckBit = 1ull << 51;
constexpr uint64_t kCancelBit = 1ull << 61;
constexpr uint64_t kClaimedBit = 1ull << 62;
constexpr uint64_t kQuitBit = 1ull << 63;
// job | n << 40 | (parts - 1) << 48 | flags (the bits above)
__host__ __device__ __forceinline__ uint64_t pack_job(uint64_t job, uint32_t n, uint32_t parts, uint64_t flags)
{
    return (job & kJobMask) | (uint64_t)n << kCountShift | (uint64_t)(parts - 1) << kPartShift | flags;
}
__host__ __device__ __forceinline__ uint64_t job_number(uint64_t w) { return w & kJobMask; }
__host__ __device__ __forceinline__ uint32_t job_count(uint64_t w) { return (uint32_t)(w >> kCountShift) & 0xFFu; }
__host__ __device__ __forceinline__ uint32_t job_parts(uint64_t w) { return (uint32_t)(w >> kPartShift & 3u) + 1u; }
// The flags: the bit itself, nonzero when set (as bool the kernel's tests of them compiled to other code).
__host__ __device__ __forceinline__ uint64_t job_write_through(uint64_t w) { return w & kWriteThroughBit; }
__host__ __device__ __forceinline__ uint64_t job_checked(uint64_t w) { return w & kCheckBit; }
__host__ __device__ __forceinline__ uint64_t job_cancelled(uint64_t w) { return w & kCancelBit; }
__host__ __device__ __forceinline__ uint64_t job_claimed(uint64_t w) { return w & kClaimedBit; }
__host__ __device__ __forceinline__ uint64_t job_quit(uint64_t w) { return w & kQuitBit; }
// Is job s of a slot finished, given the slot's done word?  Jobs of a slot run
// one at a time in number order (40-bit, wrapping), so a done word at or past
// s means s has run -- a ticket may be waited for after a later job of the
// same slot finished.
__host__ __device__ __forceinline__ bool job_done(uint64_t done, uint64_t s)
{
    return ((done - s) & kJobMask) < (1ull << 39);
}

// word + 31 slots: a slot's first 512 bytes, one 16-byte load per lane of
// wave 0 -- a cfg1 read (16 frames of 4 KiB, and a partial one) fits
constexpr int kPollDescs = 31;
static_assert(kPollDescs < 64, "one lane of wave 0 per polled slot");
constexpr uint64_t kAddrMask = (1ull << 48) - 1;
constexpr uint32_t kLenMask = (1u << 21) - 1;  // kResMaxBytes fits
static_assert(kResMaxBytes <= kLenMask, "tagged length");
__host__ __device__ __forceinline__ ResDesc tag_desc(ResDesc x, uint64_t job)
{
    x.addr |= (job & 0xFFFFull) << 48;
    x.len |= (uint32_t)(job & 0x7FFu) << 21;
    return x;
}
__host__ __device__ __forceinline__ bool desc_tagged(const ResDesc& x, uint64_t job)
{
    return (x.addr >> 48) == (job & 0xFFFFull) && (x.len >> 21) == (uint32_t)(job & 0x7FFu);
}
__host__ __device__ __forceinline__ ResDesc untag_desc(ResDesc x)
{
    x.addr &= kAddrMask;
    x.len &= kLenMask;
    return x;
}
// The verdict word (ResSlot::verdict): an address tagged like a descriptor's.
__host__ __device__ __forceinline__ uint64_t tag_verdict(uint64_t addr, uint64_t job)
{
    return addr | (job & 0xFFFFull) << 48;
}
__host__ __device__ __forceinline__ bool verdict_tagged(uint64_t v, uint64_t job)
{
    return (v >> 48) == (job & 0xFFFFull);
}
__host__ __device__ __forceinline__ uint64_t untag_verdict(uint64_t v) { return v & kAddrMask; }

// Words of a payload's 16-byte aligned hull.
__host__ __device__ __forceinline__ uint32_t hull_words(uint64_t addr, uint32_t len)
{
    return len ? (uint32_t)(((addr + len + 15) >> 4) - (addr >> 4)) : 0u;
}
// The address of word w of the job, in payload x whose first hull word is the job's word `pre`.
__host__ __device__ __forceinline__ uint64_t word_addr(const ResDesc& x, uint32_t w, uint32_t pre)
{
    return ((x.addr >> 4) + (w - pre)) << 4;
}
// The parts a job of `words` hull words runs on: one per kPartWords, at most kResParts.
__host__ __device__ __forceinline__ uint32_t part_count(uint64_t words)
{
    const uint64_t p = words / kPartWords;
    return p < 1 ? 1u : p > (uint64_t)kResParts ? (uint32_t)kResParts : (uint32_t)p;
}
// Part `part` of `parts` runs words [begin, end) of the job's `total`: an even
// share, in job order.  The kernel runs this range; the host picks each part's
// edge word with it (edge_pick).
struct PartRange { uint32_t begin, end; };
__host__ __device__ __forceinline__ PartRange part_range(uint32_t total, uint32_t part, uint32_t parts)
{
    return PartRange{(uint32_t)((uint64_t)total * part / parts), (uint32_t)((uint64_t)total * (part + 1) / parts)};
}
// A checked part is one round of the kernel (no look-back is carried between
// rounds): does the largest part of `words` over `parts` fit one?
__host__ __device__ __forceinline__ bool checked_fits(uint64_t words, uint32_t parts)
{
    return (words + parts - 1) / parts <= (uint64_t)(kResBlock * kResWords);
}
// Where the four bytes before part `part`'s first word lie: payload `index`,
// `offset` bytes past its hull's 16-byte aligned base.  index < 0: the part
// starts on a payload's first hull word (or is empty), which takes the view.
struct EdgePick { int32_t index; uint32_t offset; };
__host__ __device__ inline EdgePick edge_pick(const ResDesc* d, uint32_t n, uint32_t total, uint32_t part,
                                              uint32_t parts)
{
    const uint32_t wb = part_range(total, part, parts).begin;
    uint32_t pre = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t hw = hull_words(d[i].addr, d[i].len);
        if (wb > pre && wb < pre + hw) return EdgePick{(int32_t)i, 16u * (wb - pre) - 4u};
        pre += hw;
    }
    return EdgePick{-1, 0u};
}

// Pinned host memory.  Host-written and device-written words sit in different
// 128-byte lines.
struct alignas(256) ResSlot {
    uint64_t word;  // pack_job | cancel << 61 | claimed << 62 | quit << 63
    // A checked job: the device view of its stage's verdict bytes, tagged with
    // the job's low 16 bits in bits 48-63 like a descriptor's address.  It
    // arrives with lane 0's poll of the job word; a stale tag is read again
    // after the word.
    uint64_t verdict;
    ResDesc desc[kResMaxDescs];  // desc[i] at 16 + 16 i
    // A checked job, written by the host before the job word and read after it
    // was seen, together with the first payload loads (no round trip of their
    // own).  view[i]: Utf8View::w of payload i (look-back bits 0-23,
    // kUtf8Checked) | the index of its verdict byte << 32.  edge[p]: the four
    // bytes before part p's first word as they lay in host memory before the
    // post, still masked -- part p - 1 may have stored them unmasked by the time
    // part p runs (PieceRecEdge::edge of the launched kernel); unused where
    // the part starts on a payload's first word, which takes the view.
    uint64_t view[kResMaxDescs];
    uint64_t edge[kResParts];
    alignas(128) uint64_t done[kResParts];  // per part: last job number finished (release: its bytes visible)
    uint64_t gone[kResParts];               // per part: incarnation whose workgroup has left
    alignas(128) uint64_t pad2;
};
static_assert(offsetof(ResSlot, verdict) == 8 && offsetof(ResSlot, desc) == 16, "desc[i] at 16 + 16 i");
static_assert(kPollDescs <= kResMaxDescs && 16 * (kPollDescs + 1) == 512 && 512 <= offsetof(ResSlot, view),
              "the polled prefix: the word, the verdict word and kPollDescs descriptors, 16 bytes per lane");
static_assert(offsetof(ResSlot, done) % 128 == 0 && offsetof(ResSlot, pad2) % 128 == 0 &&
                  offsetof(ResSlot, gone) + sizeof(ResSlot::gone) <= offsetof(ResSlot, done) + 128,
              "done / gone on a 128-byte line of their own");
struct ResMailbox {
    ResSlot slot[kResSlots];
    alignas(128) uint64_t exited;  // incarnation whose last workgroup has left (device)
    alignas(128) uint64_t resize;  // (host) incarnations up to this one leave: a slot was claimed outside them
    alignas(128) uint64_t pad3;
};
// Why a workgroup left: its lease ran out, another workgroup found the grid
// idle (closing), a thread asked for a resize, it found the grid idle itself,
// its slot's quit bit.  The order kmws_resident_exit_reasons publishes.
enum ResExit : uint32_t { kExitLease = 0, kExitClosing, kExitResize, kExitIdle, kExitQuit };
constexpr int kResExitReasons = kExitQuit + 1;
// Device memory, shared by the grid's workgroups.  Counters and marks are
// compared with the incarnation number, so nothing is cleared between launches.
struct ResCtl {
    uint64_t closing;   // max incarnation that is leaving (idle or lease)
    uint64_t exits;     // workgroups exited, all incarnations (each adds the grid size)
    uint64_t idle;      // workgroups of the running incarnation idle 200 us (or gone on their quit bit)
    uint64_t pad;
    uint64_t why[kResExitReasons];  // workgroup exits by reason (kmws_resident_exit_reasons)
};

}  // namespace kmws
