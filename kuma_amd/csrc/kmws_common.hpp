// Shared device helpers for the kmws kernels (gfx950 / CDNA4, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "kmws_gpu.h"

namespace kmws {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;          // 4 waves of 64 lanes

// First 16 bytes of every workspace: status word, zeroed by a kernel (not a memset node: see launch_zero) at the
// start of each batch call.
struct WsHead {
    uint32_t status;
    uint32_t pad[3];
};
constexpr uint32_t kStatusBadDesc = 1u;
constexpr uint32_t kStatusBadHeader = 2u;
constexpr uint32_t kStatusLookbackTimeout = 4u;  // a scan predecessor never published: outputs invalid

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Mask word for an aligned dword whose first byte sits at (address - frame
// start) == -o (mod 4): byte j of the dword takes key byte (j - o) & 3, i.e.
// rotl32(key, 8*(o & 3)) with key = LE u32 of the wire key bytes.
__device__ __forceinline__ uint32_t rot_key(uint32_t key, uint64_t frame_off)
{
    return __builtin_rotateleft32(key, (uint32_t)(frame_off & 3u) * 8u);
}

// Byte-select mask for bytes [lo, hi) of dword d (0..3) of a 16-byte word.
__device__ __forceinline__ uint32_t dword_byte_mask(int lo, int hi, int d)
{
    int a = lo - 4 * d, b = hi - 4 * d;
    a = a < 0 ? 0 : a;
    b = b > 4 ? 4 : b;
    if (b <= a) return 0u;
    uint32_t hm = b >= 4 ? 0xFFFFFFFFu : ((1u << (8 * b)) - 1u);
    uint32_t lm = (1u << (8 * a)) - 1u;
    return hm & ~lm;
}

// Bytes [lo, hi) of a 16-byte word as a lane mask, 0 <= lo, hi <= 16 (empty when
// hi <= lo): two 64-bit halves, a shift and a select each, no branches.
__device__ __forceinline__ uint64_t low_bytes64(int k)  // bytes [0, k) of 8, 0 <= k <= 8
{
    return k >= 8 ? ~0ull : ((1ull << (8 * k)) - 1ull);
}
__device__ __forceinline__ u32x4 word_byte_range(int lo, int hi)
{
    const int l0 = lo < 8 ? lo : 8, h0 = hi < 8 ? hi : 8;
    const int l1 = lo > 8 ? lo - 8 : 0, h1 = hi > 8 ? hi - 8 : 0;
    const uint64_t a = low_bytes64(h0) & ~low_bytes64(l0);
    const uint64_t b = low_bytes64(h1) & ~low_bytes64(l1);
    return u32x4{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
}

// ---- unmask plan records and the block -> tile mapping (kmws_unmask.hip) ----
//
// One record per tile, written by the plan kernels and read by the apply with
// one 8-byte scalar load: the frame whose region holds the tile start, whether
// that frame's payload covers the whole tile, and if so its key already
// rotated for the tile's words.  The flag shares the index word (bit 31), which
// holds for batches of fewer than 2^31 frames; larger batches never set it and
// keep all 32 bits for the index (every tile then takes the descriptor paths).
struct alignas(8) TileRec {
    uint32_t frame;  // frame index; bit 31: covered (batches below kTileRecMaxFlagged frames)
    uint32_t rkey;   // covered: rot_key(key, off) of that frame
};
// A tile's record and the next tile's (the last tile's is the sentinel), as the apply loads them.
struct alignas(8) TileRecPair {
    TileRec at, next;
};
constexpr uint32_t kTileRecCovered = 0x80000000u;
constexpr uint32_t kTileRecMaxFlagged = 0x80000000u;  // n below this: bit 31 of `frame` is the flag
__host__ __device__ __forceinline__ bool tile_rec_covered(TileRec r, uint32_t n)
{
    return n < kTileRecMaxFlagged && (r.frame & kTileRecCovered) != 0u;
}
__host__ __device__ __forceinline__ uint32_t tile_rec_frame(TileRec r, uint32_t n)
{
    return n < kTileRecMaxFlagged ? r.frame & ~kTileRecCovered : r.frame;
}

// A placement kind as (k, c, w), all powers of two (c may be 0): blocks dealt
// over k equal parts of the span (c == 0), or the span cut into runs of c
// tiles dealt round-robin to the k residues of the block index, the residues
// in w groups that each keep their runs inside their own w-th of the span.
struct Split {
    uint32_t k, c, w;
};
// The same, prepared on the host for a span of nfull whole tiles so that the
// kernel maps a block with shifts, masks and one multiply: no division.
struct TileMapping {
    uint32_t whole;  // blocks below this are dealt; the rest take tile = block
    uint32_t part;   // tiles per part (c == 0) or per group window (c > 0)
    uint32_t lk;     // log2 k
    uint32_t lc;     // log2 c (c > 0)
    uint32_t lw;     // log2 w
    uint32_t runs;   // c > 0
};
__host__ __device__ __forceinline__ uint32_t ilog2_pow2(uint32_t x)
{
    uint32_t r = 0;
    while ((1u << r) < x) ++r;
    return r;
}
__host__ __device__ __forceinline__ TileMapping tile_mapping(uint32_t nfull, Split sp)
{
    TileMapping m;
    m.lk = ilog2_pow2(sp.k);
    m.lw = ilog2_pow2(sp.w);
    m.runs = sp.c != 0u;
    if (!m.runs) {
        m.lc = 0;
        m.part = nfull >> m.lk;
        m.whole = m.part << m.lk;
    } else {
        m.lc = ilog2_pow2(sp.c);
        const uint32_t lrun = m.lk - m.lw + m.lc;  // a group's round of runs: (k / w) * c tiles
        m.part = ((nfull >> m.lw) >> lrun) << lrun;
        m.whole = m.part << m.lw;
    }
    return m;
}
__host__ __device__ __forceinline__ uint32_t tile_of_block(uint32_t b, TileMapping m)
{
    if (b >= m.whole) return b;  // past the last whole round: the remaining tiles in order
    const uint32_t x = b & ((1u << m.lk) - 1u), i = b >> m.lk;
    if (!m.runs) return x * m.part + i;
    const uint32_t g = x & ((1u << m.lw) - 1u), xi = x >> m.lw;
    return g * m.part + ((i >> m.lc) << (m.lk - m.lw + m.lc)) + (xi << m.lc) + (i & ((1u << m.lc) - 1u));
}
__host__ __device__ __forceinline__ uint32_t tile_of_block(uint32_t b, uint32_t nfull, Split sp)
{
    return tile_of_block(b, tile_mapping(nfull, sp));
}
// Placement kind (the low byte of a schedule code, include/kmws_gpu.h) -> Split.
__host__ __device__ __forceinline__ bool split_of(uint32_t kind, Split* sp)
{
    switch (kind) {
    case KMWS_SCHED_GROUPED_RUNS: *sp = {8u, 16u, 2u}; return true;  // 2 groups of 4 XCDs, runs of 16 per half
    case KMWS_SCHED_IN_ORDER: *sp = {1u, 0u, 1u}; return true;
    case KMWS_SCHED_SPLIT2: *sp = {2u, 0u, 1u}; return true;
    case KMWS_SCHED_SPLIT8: *sp = {8u, 0u, 1u}; return true;
    case KMWS_SCHED_XCD_RUNS: *sp = {8u, 16u, 1u}; return true;
    case KMWS_SCHED_SPLIT4: *sp = {4u, 0u, 1u}; return true;
    default: return false;
    }
}

inline kmws_status hip_status(hipError_t e)
{
    return e == hipSuccess ? KMWS_OK : KMWS_ERR_FAILED;
}

// Argument tests the batch entries share.
inline bool mode_ok(int mode) { return mode == KMWS_MODE_CLIENT || mode == KMWS_MODE_SERVER; }
inline bool have_device() { static const bool have = kmws_device_count() > 0; return have; }

// Workspace carving: sizes rounded up to 16 bytes (a vector word) and to 256.
inline uint64_t r16(uint64_t x) { return (x + 15) & ~15ull; }
inline uint64_t r256(uint64_t x) { return (x + 255) & ~255ull; }

// Zeroes `bytes` (a multiple of 8, at most 4 KiB) at an 8-byte aligned device
// address with one small kernel.  Used instead of hipMemsetAsync for the status
// word and scan totals: a call captured into a HIP graph then holds kernel nodes
// only (replayed memset nodes of this runtime were seen writing a pointer value
// instead of zero when the graph was replayed after other work on the device).
kmws_status launch_zero(void* p, uint32_t bytes, hipStream_t s);

// The unmask plan (kmws_unmask.hip), for the other passes over a batch's tiles
// (kmws_utf8.hip): zeroes the workspace's WsHead, validates the descriptors
// (kStatusBadDesc) and writes one TileRec per kPlanTile bytes of [0, span), plus
// the sentinel, behind the WsHead.  KMWS_ERR_BUFFER_TOO_SMALL below
// kmws_unmask_workspace_size(span) bytes.
constexpr uint64_t kPlanTile = 16384;
kmws_status launch_plan(uint64_t span, const kmws_desc* descs, uint32_t n, void* workspace, size_t ws_bytes,
                        hipStream_t s);

// Small host batches (the decoder's staging, kmws_unmask.hip): one block per
// piece of at most kPieceWords 16-byte words of one frame's aligned hull.
constexpr uint32_t kPieceWords = 4 * kBlock;  // 16 KiB
struct PieceRec {
    uint32_t frame;  // index into the descriptor list
    uint32_t piece;  // piece of that frame's hull
};
// Pieces of a payload at byte offset `off`, `len` bytes (0 for an empty one).
inline uint64_t piece_count(uint64_t off, uint32_t len)
{
    if (len == 0) return 0;
    const uint64_t words = ((off + len + 15) >> 4) - (off >> 4);
    return (words + kPieceWords - 1) / kPieceWords;
}
// Unmasks the payloads of descs[] (device-visible, sorted or not, disjoint)
// in base[] with one launch over the np pieces; no plan, no validation (the
// caller produced the descriptors).
kmws_status launch_unmask_pieces(uint8_t* base, const kmws_desc* descs, const PieceRec* pieces, uint32_t np,
                                 hipStream_t s);

// The same launch with the UTF-8 check of kmws_decoder_set_utf8_check in its
// payload pass (kmws_utf8.hip: unmask_pieces_utf8_kernel).  views[f] belongs to
// descs[f]: w = the look-back at the frame's first payload byte | kUtf8Checked
// (0: not checked, the frame is only unmasked), slot = the index of the frame's
// byte in verdict[], which the caller zeroed and reads after the launch has
// finished: 1 = the rule rejects a byte of the frame.  A descriptor with key 0
// stores nothing to its payload (the check-only job of an unmasked frame).
// edge: the four bytes before the piece's first word as they lie in memory
// before the launch (still masked), read by the host -- another block may
// already have unmasked them when this piece's block runs; piece 0 has none.
struct Utf8View;
struct PieceRecEdge {
    uint32_t frame;
    uint32_t piece;
    uint32_t edge;
};
kmws_status launch_unmask_pieces_utf8(uint8_t* base, const kmws_desc* descs, const Utf8View* views,
                                      const PieceRecEdge* pieces, uint32_t np, uint8_t* verdict, hipStream_t s);

// KMWS_DEVICE_AUTO -> the calling thread's device (kmws_devmap.cpp; negative
// without a gfx950 device); any other value unchanged.
int resolve_device(int device);
// A device batch (an HBM-resident kernel over `bytes` of traffic) was just
// enqueued on `stream` (its device; the current device for the null stream):
// until about when it should
// have finished (queued batches add up), the resident grid on that device
// stores large jobs write-through instead of releasing the L2 once per job
// (kmws_resident.hip: kResWriteThroughWords).
void note_device_batch(uint64_t bytes, hipStream_t stream);
bool device_batch_running(int device);

// Resident worker (kmws_resident.hip): host jobs of at most kResMaxDescs
// payloads and kResMaxBytes bytes go to the calling thread's slot of a grid
// that stays on the GPU polling pinned memory, instead of a launch per call.
constexpr int kResMaxDescs = KMWS_RESIDENT_MAX_PAYLOADS;
// A job runs on up to four workgroups of its slot (one per 16 KiB of hull
// words): 256 KiB take ~11 us on the device (tools/zc_probe.hip), a launch of
// the pieces kernel alone ~20 us.  Synchronous (a flush, a feed, a mask) and
// asynchronous jobs (an rx / tx batch's submit) alike.
constexpr uint64_t kResMaxBytes = KMWS_RESIDENT_MAX_BYTES;
// A checked job (kmws_decoder_set_utf8_check) above this many bytes launches:
// the grid validates with the 16 waves of one workgroup per part, four to a
// SIMD, and the rule's ALU work no longer hides behind PCIe as it does in a
// launch's hundreds of small blocks.  Measured, one loop thread, one flush,
// grid against launch (profiles/p07_resident_utf8.json): 64 KiB (16 x 4 KiB)
// 21.7-24.7 us against 26.9-30.4 us; 256 KiB (64 x 4 KiB) 64.3-69.1 us against
// 40.8-41.3 us.  64 KiB is also the most kuma reads at once.
constexpr uint64_t kResMaxBytesChecked = KMWS_RESIDENT_MAX_CHECKED_BYTES;
struct ResidentJob {
    int device = -1;
    int slot = -1;
    uint64_t seq = 0;
};
// Posts the unmask of descs[0..n) over dev_base and descs2[0..n2) over
// dev_base2 (device views of pinned host memory, offsets relative to them) on
// the calling thread's slot and returns at once.  KMWS_ERR_NOT_SUPPORTED
// (nothing posted): too large for one job, no slot free, the thread switched
// the worker off, its slot still runs a job, or the worker is unusable -- the
// caller launches instead.
// check: the job is a checked one (kmws_decoder_set_utf8_check): the grid
// validates the payloads whose view is checked in the pass that unmasks them,
// and sets verdict_dv[view.slot] to 1 where the rule rejects a byte -- the
// contract of launch_unmask_pieces_utf8 above, key 0 included.  views: one per
// descs[] entry (nullptr: none checked); views2: for the first n_views2 entries
// of descs2[] (the rest unchecked).  A view whose slot is not below n_verdict is
// taken as unchecked.  verdict_dv: the device view of n_verdict pinned bytes,
// zeroed by the caller, which stay valid until the job is done or withdrawn.
// host_base / host_base2: the host addresses of dev_base / dev_base2 (the words
// at a part boundary are read there before the post).  KMWS_ERR_NOT_SUPPORTED
// also while the grid still runs as its unchecked instantiation: it was asked
// to leave, and the next one validates.
struct ResidentCheck {
    const Utf8View* views;
    const Utf8View* views2;
    size_t n_views2;
    uint8_t* verdict_dv;
    uint32_t n_verdict;
    const uint8_t* host_base;
    const uint8_t* host_base2;
};
kmws_status resident_post(int device, const kmws_desc* descs, const uint8_t* dev_base, size_t n,
                          const kmws_desc* descs2, const uint8_t* dev_base2, size_t n2, ResidentJob* job,
                          uint64_t max_bytes = kResMaxBytes, const ResidentCheck* check = nullptr);
// 1: done; 0: running; KMWS_ERR_NOT_SUPPORTED: withdrawn, never run (launch it).
int resident_test(const ResidentJob& job);
// KMWS_OK: done.  KMWS_ERR_NOT_SUPPORTED: withdrawn, never run (launch it).
// KMWS_ERR_TIMEOUT: neither finished nor abandoned in time -- the device may
// still write the payloads, so their memory must not be reused.
kmws_status resident_wait(const ResidentJob& job);
// post + wait.
kmws_status resident_unmask(int device, const kmws_desc* descs, const uint8_t* dev_base, size_t n,
                            const kmws_desc* descs2, const uint8_t* dev_base2, size_t n2);

}  // namespace kmws
