// Batched in-place WebSocket payload unmask for MI355X (gfx950).
//
// Replaces the per-frame scalar loop WSHandler::handleDataMask
// (src/ws/WSHandler.cpp:303-310; gate :291-301) with one stream-ordered pass
// over a whole descriptor batch.  Byte semantics are identical: payload byte
// j of a frame is XORed with maskey[j % 4]; key phase restarts per frame.
//
// Layout: the payload address space [0, span) of `base` is cut into fixed
// tiles of kTile bytes.  A prep kernel writes, for every tile, a record
// (TileRec, kmws_common.hpp): the index of the frame whose region (its offset
// up to the next frame's offset) contains the tile start, whether that frame
// covers the whole tile, and if so its rotated key -- so a tile block finds
// its frames, and a covered tile its whole mask, with one scalar load.  The main
// kernel block (256 lanes) issues its 16-byte loads first, then stages the
// descriptors of the frames overlapping its tile in LDS and builds a per-word
// mask (a rotated key splatted over the payload bytes of the word; header or
// gap bytes get 0), XORs and stores whole 16-byte words.  HBM-bound: 2 bytes
// of traffic per payload byte + 16 B per descriptor; no MFMA.
#include "kmws_common.hpp"
#include "kmws_frame_parse.hpp"
#include "kmws_unmask_tile.hpp"
#include "kmws_workspace.hpp"

namespace kmws {

// Diagnostic build only (KMWS_DIAG_PHASE_STAMPS, kuma_amd/build.py `defines`;
// loaded by path by tools/block_phases.py, never the product library): one
// apply block in 1024 keeps six s_memtime stamps in scalar registers -- entry,
// index math done, payload loads issued, metadata arrived, first payload word
// arrived, last store issued -- and writes them to a side buffer at its end.
// Stamping costs about a tenth of the wave's cycles: the record is for the
// share of each phase, not for rates.  Without the define no stamp executes.
#ifdef KMWS_DIAG_PHASE_STAMPS
constexpr int kDiagStamps = 6;
constexpr uint32_t kDiagEvery = 1024;
__device__ uint64_t* g_diag_stamps = nullptr;
__device__ uint32_t g_diag_slots = 0;
#define KMWS_STAMP(st, i)                              \
    do {                                               \
        __builtin_amdgcn_sched_barrier(0);             \
        if (st) (st)[i] = __builtin_amdgcn_s_memtime(); \
        __builtin_amdgcn_sched_barrier(0);             \
    } while (0)
#define KMWS_STAMP_AFTER(st, i, waitcnt)               \
    do {                                               \
        __builtin_amdgcn_sched_barrier(0);             \
        if (st) {                                      \
            asm volatile("s_waitcnt " waitcnt ::: "memory"); \
            (st)[i] = __builtin_amdgcn_s_memtime();    \
        }                                              \
        __builtin_amdgcn_sched_barrier(0);             \
    } while (0)
#define KMWS_STAMP_AFTER_VM(st, i, cnt)                 \
    do {                                               \
        __builtin_amdgcn_sched_barrier(0);             \
        if (st) {                                      \
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(cnt) : "memory"); \
            (st)[i] = __builtin_amdgcn_s_memtime();    \
        }                                              \
        __builtin_amdgcn_sched_barrier(0);             \
    } while (0)
#else
#define KMWS_STAMP(st, i) do { (void)(st); } while (0)
#define KMWS_STAMP_AFTER(st, i, waitcnt) do { (void)(st); } while (0)
#define KMWS_STAMP_AFTER_VM(st, i, cnt) do { (void)(st); } while (0)
#endif

// Frame f's records for the tiles [b0, b1) whose start lies in its region, and
// the sentinel after the last tile ("next tile's frame" of the last tile).  A
// tile is covered when the payload [off, off + len) holds all of it -- the
// test the apply's one-frame path made on the descriptor.
__device__ __forceinline__ void write_tile_recs(TileRec* __restrict__ map, uint32_t f, uint32_t n, uint64_t off,
                                                uint32_t len, uint32_t key, uint64_t b0, uint64_t b1,
                                                uint32_t tile_shift)
{
    const uint64_t end = off + len;
    const uint32_t r = rot_key(key, off);
    const bool flagged = n < kTileRecMaxFlagged;
    for (uint64_t b = b0; b < b1; ++b) {
        const uint64_t lo = b << tile_shift, hi = (b + 1) << tile_shift;
        const bool cov = flagged && off <= lo && end >= hi;
        map[b] = TileRec{cov ? f | kTileRecCovered : f, cov ? r : 0u};
    }
    if (f == n - 1) map[b1] = TileRec{f, 0u};
}

// Tile -> first frame map.  Frame f owns tile starts in [start_f, next_f)
// where start_0 = 0, start_f = off_f, next_f = off_{f+1} (span for the last).
// Validates sortedness / non-overlap / bounds on the fly.
__global__ void __launch_bounds__(kBlock) tile_map_kernel(const kmws_desc* __restrict__ d, uint32_t n,
                                                          uint64_t span, uint32_t tile_shift,
                                                          TileRec* __restrict__ map,
                                                          WsHead* __restrict__ head)
{
    const uint32_t f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n) return;
    const kmws_desc df = d[f];
    const uint64_t next = (f + 1 < n) ? d[f + 1].off : span;
    if (df.off > span || df.off + (uint64_t)df.len > next) {
        atomicOr(&head->status, kStatusBadDesc);
        return;
    }
    const uint64_t start = f == 0 ? 0 : df.off;
    const uint64_t T = 1ull << tile_shift;
    const uint64_t b0 = (start + T - 1) >> tile_shift;
    const uint64_t b1 = (next + T - 1) >> tile_shift;
    write_tile_recs(map, f, n, df.off, df.len, df.key, b0, b1, tile_shift);
}

// Descriptor-indexed decode and the unmask plan in one pass
// (kmws_unpack_unmask): lane f parses frame f's header (unpack_one: out_desc,
// flags, err) and writes the tile map over its region [hdr_off[f],
// hdr_off[f+1]) -- from 0 for the first frame, to the span for the last.  The
// regions partition the wire and each frame's payload lies inside its own
// (unpack_one rejects a frame that overruns the next header), so the map means
// what tile_map_kernel's does, with no 16-byte descriptor round trip and no
// second launch over the batch.  Offsets out of order or past the wire set
// kStatusBadDesc (the apply then stores nothing); a header error sets
// kStatusBadHeader and leaves that frame empty (the others are unmasked).
__global__ void __launch_bounds__(kBlock) unpack_plan_kernel(const uint8_t* __restrict__ wire, uint64_t span,
                                                             const uint64_t* __restrict__ hdr_off, uint32_t n,
                                                             int mode, kmws_desc* __restrict__ out_desc,
                                                             uint16_t* __restrict__ out_flags,
                                                             uint8_t* __restrict__ out_err, uint32_t tile_shift,
                                                             TileRec* __restrict__ map, WsHead* __restrict__ head)
{
    const uint32_t f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= n) return;
    const kmws_desc df = unpack_one(wire, span, hdr_off, n, f, mode, out_desc, out_flags, out_err, head);
    const uint64_t h = hdr_off[f];
    const uint64_t next = f + 1 < n ? hdr_off[f + 1] : span;
    if (h > next || next > span) {
        atomicOr(&head->status, kStatusBadDesc);
        return;
    }
    const uint64_t start = f == 0 ? 0 : h;
    const uint64_t T = 1ull << tile_shift;
    const uint64_t b0 = (start + T - 1) >> tile_shift;
    const uint64_t b1 = (next + T - 1) >> tile_shift;
    // df: the descriptor this lane just wrote (empty after a header error)
    write_tile_recs(map, f, n, df.off, df.len, df.key, b0, b1, tile_shift);
}

// Mask and store a loaded tile.  rec, rec_next = the plan records of the tile
// and of the one after it, ok = plan status clean; the caller loads all three
// before the payload, so that they arrive under it.
template <int V, bool FULL, bool TWO = false, bool NT = true>
__device__ __forceinline__ void finish_tile(uint8_t* __restrict__ base, uint64_t tile_lo, uint64_t tile_hi,
                                            const kmws_desc* __restrict__ d, uint32_t n, TileRec rec,
                                            TileRec rec_next, bool ok, const u32x4 (&v)[V], uint64_t* s_off,
                                            uint64_t* s_end, uint32_t* s_key, const u32x4* pre = nullptr,
                                            uint64_t* stamps = nullptr)
{
    constexpr int SP = !NT ? kPolPlain : (TWO ? kPolStreamStoreLarge : kPolStreamStoreSmall);  // TWO: the capped launches
    const int tid = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(base, tile_lo, tile_hi);
    KMWS_STAMP_AFTER(stamps, 3, "lgkmcnt(0)");  // the records and the status word are here

    // Fast path: one frame covers the whole tile (every tile of a 64 KiB-frame
    // arena).  The plan made the test and rotated the key (write_tile_recs), so
    // the record is the only metadata the block waits for: no descriptor load
    // after it.  Block-uniform scalars only: the branch needs no LDS or barrier.
    if (FULL && tile_rec_covered(rec, n)) {
        const uint32_t r = rec.rkey;
        KMWS_STAMP_AFTER(stamps, 4, "vmcnt(3)");  // the first of the V = 4 payload words is here
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint64_t a = tile_lo + 16u * (uint64_t)(tid + kBlock * i);
            if (ok) store_word<SP>(v[i] ^ r, rs, (uint32_t)(a - tile_lo));
        }
        KMWS_STAMP(stamps, 5);
        return;
    }

    // frames [f, flast] are the only ones that can overlap the tile: flast's
    // region holds the next tile's start (the map's last entry is a sentinel)
    const uint32_t f = tile_rec_frame(rec, n);
    const uint32_t flast = tile_rec_frame(rec_next, n);
    const kmws_desc d0 = d[f < n ? f : 0];

    // Two frames at most (a frame boundary inside the tile, e.g. a packed wire
    // image of frames longer than a tile): both descriptors are block-uniform
    // scalars, each word's mask is built from them directly -- no LDS, no
    // barrier (at 2-3 blocks per CU a barrier's latency is not hidden; TWO: the
    // capped launches; uncapped, the LDS path measured faster on 4 KiB frames).
    // Every mask is built before the first store, so the mask ALU runs while
    // the payload loads are still in flight (built word by word between the
    // stores, it delayed each boundary tile's stores by ~12 %: the two-frame
    // path replaced by a plain XOR ran the packed wire at the aligned rate,
    // profiles/r02bj_unmask_two_frame_ab.txt).  Words whose mask is zero (headers,
    // gaps) are not stored.
    if (TWO && FULL && flast <= f + 1 && f < n) {
        const kmws_desc d1 = flast > f && flast < n ? d[flast] : kmws_desc{~0ull, 0u, 0u};
        u32x4 m[V];
        two_frame_masks(tile_lo, d0, d1, tid, m);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint64_t a = tile_lo + 16u * (uint64_t)(tid + kBlock * i);
            if (ok && (m[i].x | m[i].y | m[i].z | m[i].w) != 0u)
                store_word<SP>(v[i] ^ m[i], rs, (uint32_t)(a - tile_lo));
        }
        return;
    }

    // General path: the descriptors of the frames overlapping the tile staged
    // in LDS, a byte-exact mask per 16-byte word (staged_masks; the first
    // round's descriptors may have been issued before the payload loads: `pre`).
    u32x4 m[V];
    staged_masks(tile_lo, tile_hi, d, n, f, flast, pre, s_off, s_end, s_key, tid, m);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint64_t a = tile_lo + 16u * (uint64_t)(tid + kBlock * i);
        const u32x4 mm = m[i];
        if (ok && (FULL || a < tile_hi) && (mm.x | mm.y | mm.z | mm.w) != 0u)
            store_word<SP>(v[i] ^ mm, rs, (uint32_t)(a - tile_lo));
    }
}

// One block for the partial last tile of a span (the split grids take the full
// tiles).  Metadata comes after the payload loads, with no early exit between
// the loads and their uses, so the compiler cannot sink the loads below the
// scalar metadata waits.  A bad plan (status != 0) stores nothing.
template <int V>
__global__ void __launch_bounds__(kBlock) unmask_tail_kernel(uint8_t* __restrict__ base, uint64_t span,
                                                             const kmws_desc* __restrict__ d, uint32_t n,
                                                             const TileRec* __restrict__ map,
                                                             const WsHead* __restrict__ head, uint32_t tile)
{
    using Cfg = UnmaskCfg<V>;
    __shared__ uint64_t s_off[Cfg::kCap];
    __shared__ uint64_t s_end[Cfg::kCap];
    __shared__ uint32_t s_key[Cfg::kCap];
    const uint64_t tile_lo = (uint64_t)tile * Cfg::kTile;
    u32x4 v[V];
    load_tile<V, false>(base, tile_lo, span, v);
    __builtin_amdgcn_sched_barrier(0);
    finish_tile<V, false>(base, tile_lo, span, d, n, map[tile], map[tile + 1], (head->status & kStatusBadDesc) == 0,
                          v, s_off, s_end, s_key);
}

// One block per full tile, blocks dealt over `k` equal parts of the span:
// block b takes tile (b mod k) * (nfull / k) + b / k, so the blocks in flight
// stream k windows far apart instead of one (the blocks past k * (nfull / k)
// take the remaining tiles in order; k = 1 is the in-order grid).  With c > 0
// the span is cut into runs of c tiles instead, dealt round-robin to the k
// residues of b (blocks go round-robin over the 8 XCDs: k = 8 gives each XCD
// its own runs).  NT: the payload store policy.
template <int V, bool TWO = false, bool NT = true>
__global__ void __launch_bounds__(kBlock) unmask_split_kernel(uint8_t* __restrict__ base,
                                                              const kmws_desc* __restrict__ d, uint32_t n,
                                                              const TileRec* __restrict__ map,
                                                              const WsHead* __restrict__ head, TileMapping tm,
                                                              uint32_t b0)
{
    using Cfg = UnmaskCfg<V>;
    __shared__ uint64_t s_off[Cfg::kCap];
    __shared__ uint64_t s_end[Cfg::kCap];
    __shared__ uint32_t s_key[Cfg::kCap];
#ifdef KMWS_DIAG_PHASE_STAMPS
    uint64_t st[kDiagStamps] = {};
#else
    uint64_t* const st = nullptr;
#endif
    KMWS_STAMP(st, 0);
    const uint32_t tile = tile_of_block(b0 + blockIdx.x, tm);
    const uint64_t lo = (uint64_t)tile * Cfg::kTile;
    // The tile's two records and the status word go out together, ahead of the
    // payload loads (scalar loads count on lgkmcnt, the payload on vmcnt: neither
    // queue holds the other up), and are waited for once, after the payload is
    // in flight.  A covered tile then needs nothing more before its stores.
    const TileRecPair recs = *reinterpret_cast<const TileRecPair*>(map + tile);  // one 16-byte scalar load
    const TileRec rec = recs.at, rec_next = recs.next;
    const uint32_t status = head->status;
    u32x4 v[V];
    if constexpr (!TWO) {
        // the tile's descriptors first: their wait then counts only them, not the
        // payload loads issued after them (vmcnt is one in-order queue; cfg4's
        // in-place unmask 80.3-80.4 -> 81.7-82.2 %,
        // profiles/r02bt_unmask_desc_prefetch_ab.txt)
        const uint32_t f = tile_rec_frame(rec, n), fl = tile_rec_frame(rec_next, n);
        const uint32_t fi = f + threadIdx.x;
        u32x4 pre = u32x4{0, 0, 0, 0};
        if (fi < n && fi <= fl) pre = *reinterpret_cast<const u32x4*>(d + fi);
        load_tile<V, true>(base, lo, lo + Cfg::kTile, v);
        __builtin_amdgcn_sched_barrier(0);
        finish_tile<V, true, TWO, NT>(base, lo, lo + Cfg::kTile, d, n, rec, rec_next,
                                      (status & kStatusBadDesc) == 0, v, s_off, s_end, s_key, &pre);
        return;
    }
    __builtin_amdgcn_sched_barrier(0);
    KMWS_STAMP(st, 1);
    if constexpr (kUnmaskDepth < V) {
        // Staged loads (kUnmaskDepth, kmws_unmask_tile.hpp): the first D words go
        // out here; a covered tile then runs word by word -- word i is waited
        // for, load i + D issued, word i stored.  The load goes out ahead of the
        // store: vmcnt is one in-order queue, so the wait for a load issued
        // after a store would also wait for that store's acknowledgement.  Any
        // other tile issues the rest at once and takes finish_tile's paths.  A
        // bad plan issues no more loads and stores nothing; the D in flight
        // drain before the wave ends.  The sched_barriers pin load / store
        // order between the steps; inside the up-front group the compiler is
        // free (at D = 3 it issues word 1's load ahead of word 0's, so the first
        // wait covers both: the stream profiles/p04_unmask_depth_ab.txt measured).
        constexpr int D = kUnmaskDepth;
        constexpr int SP = NT ? kPolStreamStoreLarge : kPolPlain;
        const __amdgpu_buffer_rsrc_t rs = tile_rsrc(base, lo, lo + Cfg::kTile);
        const bool ok = (status & kStatusBadDesc) == 0;
        load_tile_words<V>(rs, v, 0, D);
        __builtin_amdgcn_sched_barrier(0);
        KMWS_STAMP(st, 2);
        if (!tile_rec_covered(rec, n)) {
            load_tile_words<V>(rs, v, D, V);
            __builtin_amdgcn_sched_barrier(0);
            finish_tile<V, true, TWO, NT>(base, lo, lo + Cfg::kTile, d, n, rec, rec_next, ok, v, s_off, s_end, s_key);
            return;
        }
        KMWS_STAMP_AFTER(st, 3, "lgkmcnt(0)");  // the records and the status word are here
        if (ok) {
            const uint32_t r = rec.rkey;
            const uint32_t x0 = 16u * (uint32_t)threadIdx.x;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (i == 0) KMWS_STAMP_AFTER_VM(st, 4, D - 1);  // the first payload word is here
                const u32x4 w = v[i] ^ r;  // the compiler's wait for word i sits here
                __builtin_amdgcn_sched_barrier(0);
                load_tile_words<V>(rs, v, i + D, i + D + 1);
                __builtin_amdgcn_sched_barrier(0);
                store_word<SP>(w, rs, x0 + 16u * (uint32_t)(kBlock * i));
                __builtin_amdgcn_sched_barrier(0);
            }
            KMWS_STAMP(st, 5);
        }
    } else {
        load_tile<V, true>(base, lo, lo + Cfg::kTile, v);
        __builtin_amdgcn_sched_barrier(0);
        KMWS_STAMP(st, 2);
        finish_tile<V, true, TWO, NT>(base, lo, lo + Cfg::kTile, d, n, rec, rec_next, (status & kStatusBadDesc) == 0,
                                      v, s_off, s_end, s_key, nullptr, st);
    }
#ifdef KMWS_DIAG_PHASE_STAMPS
    const uint32_t blk = b0 + blockIdx.x;
    if (blk % kDiagEvery == 0 && blk / kDiagEvery < g_diag_slots && threadIdx.x == 0 && st[5] != 0)
        for (int i = 0; i < kDiagStamps; ++i) g_diag_stamps[(uint64_t)(blk / kDiagEvery) * kDiagStamps + i] = st[i];
#endif
}

// Small host batches: the decoder's payloads of one socket read or one loop
// iteration, produced by its own parser (disjoint, in range: nothing to
// validate).  A plan + apply per read costs more than the bytes, so these go
// in ONE launch: block b unmasks piece pieces[b] -- up to kPieceWords words of
// one frame's aligned hull -- with descriptors and piece list read from
// host-visible memory.  A hull's first and last words may hold bytes of other
// frames (or headers): those words are written byte by byte, the frame's own
// bytes only, so blocks of neighbouring frames never write the same byte.
__global__ void __launch_bounds__(kBlock) unmask_pieces_kernel(uint8_t* __restrict__ base,
                                                               const kmws_desc* __restrict__ d,
                                                               const PieceRec* __restrict__ pieces)
{
    constexpr int V = kPieceWords / kBlock;
    const PieceRec pr = pieces[blockIdx.x];
    const kmws_desc x = d[pr.frame];
    const PieceHull h = piece_hull(x, pr.piece);
    u32x4 v[V];
    load_piece(base, h, v);
    store_piece(base, x, h, v);
}

// Blocks of an apply grid resident per CU, chosen together with the load depth
// kUnmaskDepth (kmws_unmask_tile.hpp) as one pair (blocks, depth).  With every
// load of a tile issued up front (depth 4) fewer blocks stream HBM better: 2
// blocks of 256 lanes per CU ran the 64 GiB batch at 84.5-84.8 % of peak against
// 82.4-82.9 % with the 6 the registers allow, 3 blocks at 83.4 %, 1 block at
// 65-75 % (profiles/r02ag_unmask_occupancy.txt).  With staged loads the best
// pairs are (3, 3), (4, 1) and (3, 2): 20.18-20.39 / 20.22-20.36 / 20.27-20.44 ms
// against 20.59-20.74 for (2, 4), the pair before; (3, 3) is the one that also
// gains on the packed wire under the default schedule
// (profiles/p04_unmask_depth_ab.txt).  The cap is dynamic LDS the kernel does
// not use: a block asks for just over a quarter of the CU's LDS.
constexpr unsigned kUnmaskBlocksPerCu = 3;

// Dynamic LDS that lets exactly `blocks_per_cu` blocks of `static_lds` bytes of
// static LDS share a CU (0 if the device cannot be asked).
unsigned lds_pad_for(unsigned blocks_per_cu, unsigned static_lds)
{
    static thread_local int dev_cached = -1;
    static thread_local unsigned lds_cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev != dev_cached) {
        int lds = 0;
        lds_cached = 0;
        if (
            hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess &&
            lds > 0)
            lds_cached = (unsigned)lds;
        dev_cached = dev;
    }
    if (!lds_cached) return 0;
    const unsigned per_block = lds_cached / (blocks_per_cu + 1) + 1;  // one more does not fit
    return per_block > static_lds ? per_block - static_lds : 0u;
}

// The cap pays where tiles take the one- or two-frame paths (regions of a tile
// or more: 16 KiB frames ran 85.5 % capped vs 79-83 % uncapped); batches of
// smaller frames (several per tile: the LDS-staged path, whose barriers need the
// latency hiding of a full CU) keep every block: 8 KiB frames ran 54.8 % capped
// vs 83 %, 4 KiB frames 47.6 % vs 80 % (profiles/r02at_unmask_framelen_occupancy.txt).
// Mean region >= 1 tile selects.
bool unmask_capped(uint64_t span, uint32_t n) { return n && span / n >= ProdCfg::kTile; }

static unsigned unmask_lds_pad(uint64_t span, uint32_t n)
{
    return unmask_capped(span, n) ? lds_pad_for(kUnmaskBlocksPerCu, kUnmaskStaticLds) : 0u;
}

// The plan's tile index is 31 bits; the workspace holds the plan.
static kmws_status plan_fits(const PlanWs& w, size_t ws_bytes)
{
    if (w.ntiles > 0x7FFFFFFFull) return KMWS_ERR_INVALID_PARAM;
    return ws_bytes < w.total ? KMWS_ERR_BUFFER_TOO_SMALL : KMWS_OK;
}

static_assert(ProdCfg::kTile == kPlanTile, "the plan's tile is the apply's");

kmws_status launch_plan(uint64_t span, const kmws_desc* descs, uint32_t n, void* workspace, size_t ws_bytes,
                        hipStream_t s)
{
    const PlanWs w = plan_ws(span);
    const kmws_status st = plan_fits(w, ws_bytes);
    if (st != KMWS_OK) return st;
    WsHead* head = at<WsHead>(workspace, 0);
    if (launch_zero(head, sizeof(WsHead), s) != KMWS_OK) return KMWS_ERR_FAILED;
    if (n == 0 || span == 0) return KMWS_OK;
    hipLaunchKernelGGL(tile_map_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, descs, n, span,
                       ilog2_pow2((uint32_t)ProdCfg::kTile), at<TileRec>(workspace, w.map), head);
    return hip_status(hipGetLastError());
}

// ---- schedules: where the blocks in flight are, and the store policy ----
//
// The tile kernel is the same for every schedule; what differs is which tiles
// the ~512 resident blocks stream at once (the in-order grid streams one 16 MiB
// window: 74.5-75 % of HBM peak everywhere; dealing blocks over far-apart parts
// of the span streams several windows: 82-86 % on some placements in physical
// HBM, 76 % on others; runs of 16 tiles per XCD hold 78-79 % on every placement;
// profiles/r01f_unmask_placement.txt, r02al_unmask_schedules_2bpc.txt) and how the
// payload is stored (non-temporal by default; see store_word).
//
// The library keeps no schedule state: kmws_unmask_autotune returns the code it
// picked for the batch it timed, and the caller passes it to
// kmws_unmask_apply_sched for that batch (the caller's plan object owns it;
// kuma_amd/kmws.py keeps it on the Workspace).  kmws_unmask_apply and
// kmws_unmask_batch use the default, by the mean region (the same test as the
// occupancy cap): split 4 for regions of a tile or more -- the best on
// plain allocations of the aligned arena (0.82), the packed wire (0.82) and
// cfg3's Zipf wire (0.81) -- and grouped XCD runs below -- the best on 4 KiB
// fragments (0.81 vs 0.78 for split 4)
// (profiles/r03m_unmask_schedule_sweep_plain_nt_fixed.jsonl); non-temporal
// stores.  The reference's handleDataMask (WSHandler.cpp:303-310) is stateless;
// so is every batch that was not tuned.
// The block -> tile mapping of a kind (Split, split_of, tile_of_block) is in
// kmws_common.hpp: the host prepares it per launch, the kernel applies it.
constexpr uint32_t kKindMask = 0xFFu;
constexpr uint32_t kSchedTemporal = KMWS_SCHED_TEMPORAL_STORES;
constexpr uint32_t kSchedNT = KMWS_SCHED_NT_STORES;
uint32_t default_schedule(uint64_t span, uint32_t n)
{
    return n && span / n >= ProdCfg::kTile ? KMWS_SCHED_SPLIT4 : KMWS_SCHED_GROUPED_RUNS;
}

bool decode_schedule(uint32_t code, Schedule* out)
{
    const uint32_t store = code & (kSchedTemporal | kSchedNT);
    out->temporal = (code & kSchedTemporal) != 0;
    return split_of(code & kKindMask, &out->split) && store != (kSchedTemporal | kSchedNT) &&
           (code & ~(kKindMask | kSchedTemporal | kSchedNT)) == 0;
}

kmws_status launch_apply(const Schedule& sc, uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                         const void* workspace, size_t ws_bytes, hipStream_t s)
{
    const PlanWs w = plan_ws(span);
    const kmws_status st = plan_fits(w, ws_bytes);
    if (st != KMWS_OK) return st;
    if (n == 0 || span == 0) return KMWS_OK;
    const WsHead* head = at<const WsHead>(workspace, 0);
    const TileRec* map = at<const TileRec>(workspace, w.map);
    const uint64_t nfull = span / ProdCfg::kTile;
    const unsigned lds_pad = unmask_lds_pad(span, n);
    const TileMapping tm = tile_mapping((uint32_t)nfull, sc.split);
    launch_split_grid(nfull, lds_pad, sc.temporal, [&](auto two, auto nt, dim3 grid, uint32_t b0, unsigned pad) {
        hipLaunchKernelGGL((unmask_split_kernel<kUnmaskV, decltype(two)::value, decltype(nt)::value>), grid,
                           dim3(kBlock), pad, s, base, descs, n, map, head, tm, b0);
    });
    if (w.ntiles > nfull)  // the partial last tile
        hipLaunchKernelGGL(unmask_tail_kernel<kUnmaskV>, dim3(1), dim3(kBlock), 0, s, base, span, descs, n, map, head,
                           (uint32_t)nfull);
    return hip_status(hipGetLastError());
}

static bool bad_args(const uint8_t* base, const kmws_desc* descs, uint32_t n, const void* ws)
{
    return !ws || (n && (!base || !descs)) || (reinterpret_cast<uintptr_t>(base) & 15u);
}

__global__ void __launch_bounds__(64) zero_kernel(uint64_t* __restrict__ p, uint32_t words)
{
    for (uint32_t i = threadIdx.x; i < words; i += 64) p[i] = 0;
}

kmws_status launch_zero(void* p, uint32_t bytes, hipStream_t s)
{
    if (!p || (bytes & 7u) || bytes > 4096) return KMWS_ERR_INVALID_PARAM;
    hipLaunchKernelGGL(zero_kernel, dim3(1), dim3(64), 0, s, static_cast<uint64_t*>(p), bytes / 8);
    return hip_status(hipGetLastError());
}

kmws_status launch_unmask_pieces(uint8_t* base, const kmws_desc* descs, const PieceRec* pieces, uint32_t np,
                                 hipStream_t s)
{
    if (np == 0) return KMWS_OK;
    if (!base || !descs || !pieces) return KMWS_ERR_INVALID_PARAM;
    hipLaunchKernelGGL(unmask_pieces_kernel, dim3(np), dim3(kBlock), 0, s, base, descs, pieces);
    return hip_status(hipGetLastError());
}

kmws_status launch_unpack_plan(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                               kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err, void* workspace,
                               hipStream_t s)
{
    WsHead* head = at<WsHead>(workspace, 0);
    if (launch_zero(head, sizeof(WsHead), s) != KMWS_OK) return KMWS_ERR_FAILED;
    if (n == 0) return KMWS_OK;
    hipLaunchKernelGGL(unpack_plan_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, wire, wire_len, hdr_off,
                       n, mode, out_desc, out_flags, out_err, ilog2_pow2((uint32_t)ProdCfg::kTile),
                       at<TileRec>(workspace, plan_ws(wire_len).map), head);
    return hip_status(hipGetLastError());
}
}  // namespace kmws

using namespace kmws;

extern "C" {

size_t kmws_unmask_workspace_size(uint64_t span)
{
    return plan_ws(span).total;
}

kmws_status kmws_unmask_batch(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                              void* workspace, size_t workspace_bytes, void* stream)
{
    if (bad_args(base, descs, n, workspace)) return KMWS_ERR_INVALID_PARAM;
    kmws_status st = launch_plan(span, descs, n, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
    if (st != KMWS_OK) return st;
    return kmws_unmask_apply(base, span, descs, n, workspace, workspace_bytes, stream);
}

kmws_status kmws_unmask_plan(uint64_t span, const kmws_desc* descs, uint32_t n, void* workspace,
                             size_t workspace_bytes, void* stream)
{
    if (!workspace || (n && !descs)) return KMWS_ERR_INVALID_PARAM;
    return launch_plan(span, descs, n, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

kmws_status kmws_unmask_apply(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                              const void* workspace, size_t workspace_bytes, void* stream)
{
    return kmws_unmask_apply_sched(base, span, descs, n, workspace, workspace_bytes, -1, stream);
}

kmws_status kmws_unmask_apply_sched(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                                    const void* workspace, size_t workspace_bytes, int schedule, void* stream)
{
    if (bad_args(base, descs, n, workspace)) return KMWS_ERR_INVALID_PARAM;
    const uint32_t code = schedule < 0 ? default_schedule(span, n) : (uint32_t)schedule;
    kmws::note_device_batch(2 * span, static_cast<hipStream_t>(stream));
    Schedule sc;
    if (!decode_schedule(code, &sc)) return KMWS_ERR_INVALID_PARAM;
    return launch_apply(sc, base, span, descs, n, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int kmws_unmask_default_schedule(uint64_t span, uint32_t n) { return (int)default_schedule(span, n); }

kmws_status kmws_unpack_unmask(uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                               kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err, void* workspace,
                               size_t workspace_bytes, int schedule, void* stream)
{
    if (bad_args(wire, out_desc, n, workspace) || (n && !hdr_off) || !mode_ok(mode)) return KMWS_ERR_INVALID_PARAM;
    Schedule sc;
    if (!decode_schedule(schedule < 0 ? default_schedule(wire_len, n) : (uint32_t)schedule, &sc))
        return KMWS_ERR_INVALID_PARAM;
    kmws_status st = plan_fits(plan_ws(wire_len), workspace_bytes);
    if (st != KMWS_OK) return st;
    hipStream_t s = static_cast<hipStream_t>(stream);
    st = launch_unpack_plan(wire, wire_len, hdr_off, n, mode, out_desc, out_flags, out_err, workspace, s);
    if (st != KMWS_OK || n == 0) return st;
    kmws::note_device_batch(2 * wire_len, s);
    return launch_apply(sc, wire, wire_len, out_desc, n, workspace, workspace_bytes, s);
}

// Times each schedule on the caller's batch, two launches per timing (XOR
// applied twice is the identity, so the payload is unchanged on return): one
// warm-up round over every schedule, then two timed rounds; a schedule's time
// is the lower of its two (one round alone let a 0.3 ms outlier pick a slower
// schedule, profiles/p01_unmask_tilerec_policy_ab.txt section 5).  Returns the
// fastest; nothing is recorded.  Synchronizes.
int kmws_unmask_autotune(uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n, void* workspace,
                         size_t workspace_bytes, void* stream)
{
    if (bad_args(base, descs, n, workspace)) return KMWS_ERR_INVALID_PARAM;
    hipStream_t s = static_cast<hipStream_t>(stream);
    kmws_status st = launch_plan(span, descs, n, workspace, workspace_bytes, s);
    if (st != KMWS_OK) return st;
    // every placement kind x both store policies: which wins depends on where the
    // batch lies in HBM, on its frame layout and on the blocks in flight
    static const uint32_t kinds[] = {KMWS_SCHED_GROUPED_RUNS, KMWS_SCHED_SPLIT4, KMWS_SCHED_SPLIT8,
                                     KMWS_SCHED_XCD_RUNS,     KMWS_SCHED_SPLIT2, KMWS_SCHED_IN_ORDER};
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess) return KMWS_ERR_FAILED;
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return KMWS_ERR_FAILED;
    }
    constexpr int kKinds = sizeof(kinds) / sizeof(kinds[0]);
    static const uint32_t stores[2] = {kSchedNT, kSchedTemporal};
    float t_min[kKinds][2];
    for (auto& t : t_min) t[0] = t[1] = 1e30f;
    for (int rep = 0; rep < 3 && st == KMWS_OK; ++rep) {
        for (int ki = 0; ki < kKinds; ++ki) {
            for (int si = 0; si < 2; ++si) {
                Schedule sc;
                (void)decode_schedule(kinds[ki] | stores[si], &sc);
                if (hipEventRecord(e0, s) != hipSuccess) { st = KMWS_ERR_FAILED; break; }
                for (int k = 0; k < 2 && st == KMWS_OK; ++k)
                    st = launch_apply(sc, base, span, descs, n, workspace, workspace_bytes, s);
                if (st != KMWS_OK || hipEventRecord(e1, s) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) {
                    st = st != KMWS_OK ? st : KMWS_ERR_FAILED;
                    break;
                }
                float ms = 0;
                (void)hipEventElapsedTime(&ms, e0, e1);
                if (rep > 0 && ms < t_min[ki][si]) t_min[ki][si] = ms;  // rep 0 warms every schedule up
            }
            if (st != KMWS_OK) break;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (st != KMWS_OK) return st;
    float best = 1e30f;
    uint32_t pick = default_schedule(span, n);
    for (int ki = 0; ki < kKinds; ++ki)
        for (int si = 0; si < 2; ++si)
            if (t_min[ki][si] < best) {
                best = t_min[ki][si];
                pick = kinds[ki] | stores[si];
            }
    return (int)pick;
}

kmws_status kmws_read_status(const void* workspace, uint32_t* status_out, void* stream)
{
    if (!workspace || !status_out) return KMWS_ERR_INVALID_PARAM;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(status_out, workspace, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return hip_status(e);
}

#ifdef KMWS_DIAG_PHASE_STAMPS
// Diagnostic build only: the side buffer of the block-phase stamps, `slots`
// records of kDiagStamps u64 each (slot = block index / kDiagEvery); null stops
// the stamping blocks from writing.  Synchronizes.
kmws_status kmws_diag_set_stamps(uint64_t* buf, uint32_t slots)
{
    const uint32_t s = buf ? slots : 0u;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_diag_slots), &s, sizeof(s)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_diag_stamps), &buf, sizeof(buf)) != hipSuccess)
        return KMWS_ERR_FAILED;
    return hip_status(hipDeviceSynchronize());
}
#endif

int kmws_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int good = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
    }
    return good;
}

}  // extern "C"
