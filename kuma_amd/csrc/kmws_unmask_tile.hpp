// Tile loads and stores of the in-place payload passes (kmws_unmask.hip, and the
// fused unmask + UTF-8 pass of kmws_utf8.hip), their mask builders, the pieces
// kernels' load and store, and what the host side of those passes shares: the
// schedule codes, the occupancy cap of the apply and the split-grid launch.
#pragma once
#include <type_traits>

#include "kmws_common.hpp"

namespace kmws {

// Payload store of a tile word: streaming (the default, and what
// KMWS_SCHED_NT_STORES asks for) or temporal (plain: the line stays in L2 and
// is written back on eviction).  The streaming store of the capped launches is
// `nt sc1`: sc1 stores drop the line from the XCD's L2 where plain, sc0 and nt
// stores keep it, and on the 64 GiB aligned batch `nt sc1` ran 20.57-20.58 ms
// against 20.65-20.66 for `nt`, with `sc1` and `sc0 sc1` alone behind both
// (20.81-20.85); every other load policy than `nt` lost or tied (`nt sc1`
// loads 20.65-20.67, `sc1` and `sc0 sc1` loads 21.95-21.99); the stand-alone
// probe (tools/policy_probe.hip) ranks the stores the same way.  The packed
// wire gained too (20.71-20.80 against 21.04-21.14 ms tuned).  Batches of
// several frames per tile keep `nt`: with `nt sc1` cfg3's Zipf wire lost
// (2.70-2.72 against 2.655 ms) where 4 KiB fragments gained (5.22-5.25 against
// 5.27), and a default must not lose on either
// (profiles/p01_unmask_tilerec_policy_ab.txt).
// On plain allocations non-temporal stores ran ahead of temporal on every layout -- the
// aligned arena 0.82 vs 0.76, the packed wire 0.82 vs 0.76, 4 KiB fragments
// 0.81 vs 0.76, cfg3's Zipf wire 0.81 vs 0.75 of peak
// (profiles/r03m_unmask_schedule_sweep_plain_nt_fixed.jsonl) -- so temporal
// stores are only a candidate of the per-batch autotune (round 2 saw them
// win by 0.3-1 point on one placed aligned arena, r02bz_unmask_store_policy_ab.txt).
// The policy is a template parameter of the apply grid, chosen on the host.
// The stores are buffer stores through a per-tile resource with the cache
// policy as an immediate: written as `if (nt) __builtin_nontemporal_store(..)
// else *p = ..`, the compiler had merged the two and dropped the hint.
// Buffer cache-policy immediates (gfx950): bit 0 sc0, bit 1 nt, bit 4 sc1.
constexpr int kPolPlain = 0, kPolNT = 2, kPolNTSC1 = 18;
// What KMWS_SCHED_NT_STORES and the default policy emit: `nt sc1` in the capped
// launches (mean region of a tile or more: nearly every line is written whole),
// `nt` in the others (several frames per tile: words of headers and gaps are
// skipped, lines are written in part).
constexpr int kPolStreamStoreLarge = kPolNTSC1;
constexpr int kPolStreamStoreSmall = kPolNT;
constexpr int kPolStreamLoad = kPolNT;  // every payload load
constexpr int kBufferRsrcWord3 = 0x00020000;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(uint8_t* base, uint64_t lo, uint64_t hi)
{
    return __builtin_amdgcn_make_buffer_rsrc(base + lo, (short)0, (int)((hi - lo + 15) & ~15ull), kBufferRsrcWord3);
}

template <int POL>
__device__ __forceinline__ void store_word(const u32x4& val, __amdgpu_buffer_rsrc_t rs, uint32_t off)
{
    __builtin_amdgcn_raw_buffer_store_b128(val, rs, (int)off, 0, POL);
}

// Each lane owns V consecutive-block words: word w = tid + kBlock * i.
template <int V>
struct UnmaskCfg {
    static constexpr int kWords = kBlock * V;
    static constexpr uint64_t kTile = (uint64_t)kWords * 16u;
    static constexpr int kCap = kBlock;  // descriptors staged per LDS round
};

// Issue every payload load of a tile.  Full tiles load unconditionally so the
// loads stay back to back.  Payload is touched once: non-temporal loads and
// stores (measured +6 % on MI355X for this in-place stream, tools/membw_probe.hip).
// Buffer loads through the tile's resource, the cache policy a template
// immediate like the stores' (as fast as the global `nt` loads they replaced:
// 20.65-20.66 ms both, profiles/p01_unmask_tilerec_policy_ab.txt).
template <int V, bool FULL, int POL = kPolStreamLoad>
__device__ __forceinline__ void load_tile(uint8_t* __restrict__ base, uint64_t tile_lo, uint64_t tile_hi,
                                          u32x4 (&v)[V])
{
    const int tid = threadIdx.x;
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(base, tile_lo, tile_hi);  // the stores' resource
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint32_t x = 16u * (uint32_t)(tid + kBlock * i);
        if (FULL || tile_lo + x < tile_hi) v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)x, 0, POL);
        else v[i] = u32x4{0, 0, 0, 0};
    }
}

// Words [I0, I1) of a full tile, back to back: the staged apply of the capped
// launches issues a tile's loads in two parts (kUnmaskDepth).
template <int V, int POL = kPolStreamLoad>
__device__ __forceinline__ void load_tile_words(__amdgpu_buffer_rsrc_t rs, u32x4 (&v)[V], int i0, int i1)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < V; ++i)
        if (i >= i0 && i < i1)
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(16u * (uint32_t)(tid + kBlock * i)), 0, POL);
}

// ---- per-word masks of a tile: the apply's and the fused pass's two builders ----
//
// Two frames at most overlap the tile (d1.off == ~0: no second frame): both
// descriptors are block-uniform scalars and each word's mask is built from them
// directly, no LDS, no barrier.  What the build leaves besides m[]: the rotated
// keys and each payload's extent relative to the tile, clamped to [0, kTile].
struct TwoFrameMasks {
    uint32_t r0, r1;  // rot_key of each frame
    uint32_t s0, t0;  // frame 0's payload bytes of the tile: [s0, t0)
    uint32_t s1, t1;  // frame 1's (empty without one)
};
template <int V>
__device__ __forceinline__ TwoFrameMasks two_frame_masks(uint64_t tile_lo, const kmws_desc& d0, const kmws_desc& d1,
                                                         int tid, u32x4 (&m)[V])
{
    TwoFrameMasks e;
    e.r0 = rot_key(d0.key, d0.off);
    e.r1 = rot_key(d1.key, d1.off);
    // block-uniform scalars, so each per-word test is one 32-bit compare
    constexpr uint32_t T = (uint32_t)UnmaskCfg<V>::kTile;
    auto rel = [&](uint64_t x) -> uint32_t {
        return x <= tile_lo ? 0u : (x - tile_lo >= T ? T : (uint32_t)(x - tile_lo));
    };
    e.s0 = rel(d0.off), e.t0 = rel(d0.off + d0.len);
    e.s1 = rel(d1.off), e.t1 = d1.len ? rel(d1.off + d1.len) : e.s1;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint32_t x = 16u * (uint32_t)(tid + kBlock * i);
        u32x4 mm = u32x4{0, 0, 0, 0};
        if (e.s0 <= x && e.t0 >= x + 16) {
            mm = u32x4{e.r0, e.r0, e.r0, e.r0};
        } else if (e.s1 <= x && e.t1 >= x + 16) {
            mm = u32x4{e.r1, e.r1, e.r1, e.r1};
        } else {  // a word holding a frame edge: byte-exact
            // each frame's bytes of the word, clamped to [0, 16] (empty if none)
            auto cl = [&](uint32_t y) -> int { return y <= x ? 0 : (y - x >= 16u ? 16 : (int)(y - x)); };
            mm = (word_byte_range(cl(e.s0), cl(e.t0)) & e.r0) | (word_byte_range(cl(e.s1), cl(e.t1)) & e.r1);
        }
        m[i] = mm;
    }
    return e;
}

// Any number of frames: the descriptors of frames [f, flast] -- the only ones
// that can overlap the tile -- are staged in LDS, kCap per round, and every
// 16-byte word gets a byte-exact mask (header and gap bytes 0).  pre: lane tid's
// descriptor f + tid of the first round, loaded by the caller ahead of the
// payload (nullptr: loaded here; then no wait here covers the payload).  Two
// barriers per round; on return every lane is done with the LDS.
template <int V>
__device__ __forceinline__ void staged_masks(uint64_t tile_lo, uint64_t tile_hi, const kmws_desc* d,
                                             uint32_t n, uint32_t f, uint32_t flast, const u32x4* pre,
                                             uint64_t* s_off, uint64_t* s_end, uint32_t* s_key, int tid,
                                             u32x4 (&m)[V])
{
    using Cfg = UnmaskCfg<V>;
    // built in a local array and handed over at the end: ORed straight into the
    // caller's m[], every kernel that inlines this came out with more copies
    u32x4 acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = u32x4{0, 0, 0, 0};
    // One round: lane tid holds descriptor f + tid (`have`: it exists and can
    // overlap the tile); returns how many were staged.
    auto round = [&](bool have, const u32x4& x) -> int {
        int valid = 0;
        if (have) {
            const uint64_t off = (uint64_t)x.x | ((uint64_t)x.y << 32);
            if (off < tile_hi) {
                valid = 1;
                s_off[tid] = off;
                s_end[tid] = off + x.z;
                s_key[tid] = x.w;
            }
        }
        const int cnt = __syncthreads_count(valid);  // sorted => a prefix
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint64_t a = tile_lo + 16u * (uint64_t)(tid + kBlock * i);
            int lo = 0, hi = cnt;  // first staged frame with end > a
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_end[mid] <= a) lo = mid + 1; else hi = mid;
            }
            for (int j = lo; j < cnt; ++j) {
                const uint64_t o = s_off[j];
                if (o >= a + 16) break;
                const uint64_t e = s_end[j];
                const uint32_t r = rot_key(s_key[j], o);
                if (o <= a && e >= a + 16) {
                    acc[i] |= u32x4{r, r, r, r};
                } else {
                    const int blo = o > a ? (int)(o - a) : 0;
                    const int bhi = e < a + 16 ? (int)(e - a) : 16;
                    acc[i].x |= r & dword_byte_mask(blo, bhi, 0);
                    acc[i].y |= r & dword_byte_mask(blo, bhi, 1);
                    acc[i].z |= r & dword_byte_mask(blo, bhi, 2);
                    acc[i].w |= r & dword_byte_mask(blo, bhi, 3);
                }
            }
        }
        __syncthreads();  // every lane done reading this round's LDS (also before a next tile reuses it)
        return cnt;
    };
    // no descriptor loads past the tile's last frame
    auto have_f = [&]() { return f + (uint32_t)tid < n && f + (uint32_t)tid <= flast; };
    auto load_f = [&]() { return have_f() ? *reinterpret_cast<const u32x4*>(d + f + tid) : u32x4{0, 0, 0, 0}; };
    int cnt = pre ? round(have_f(), *pre) : round(have_f(), load_f());
    while (cnt == Cfg::kCap) {
        f += Cfg::kCap;
        cnt = round(have_f(), load_f());
    }
#pragma unroll
    for (int i = 0; i < V; ++i) m[i] = acc[i];
}

// ---- pieces of one frame's aligned hull (unmask_pieces_kernel, kmws_unmask.hip;
// unmask_pieces_utf8_kernel, kmws_utf8.hip): V = kPieceWords / kBlock words per
// lane, word w0 + tid + kBlock * i ----
struct PieceHull {
    uint64_t w0, w1;  // the piece's 16-byte words: [w0, w1)
    uint64_t end;     // the payload's end
    uint32_t r;       // its rotated key
};
__device__ __forceinline__ PieceHull piece_hull(const kmws_desc& x, uint32_t piece)
{
    PieceHull h;
    h.end = x.off + x.len;
    h.w0 = (x.off >> 4) + (uint64_t)piece * kPieceWords;
    const uint64_t wh = (h.end + 15) >> 4;
    h.w1 = wh < h.w0 + kPieceWords ? wh : h.w0 + kPieceWords;
    h.r = rot_key(x.key, x.off);
    return h;
}
template <int V>
__device__ __forceinline__ void load_piece(const uint8_t* __restrict__ base, const PieceHull& h, u32x4 (&v)[V])
{
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint64_t w = h.w0 + threadIdx.x + (uint64_t)kBlock * i;
        v[i] = w < h.w1 ? *reinterpret_cast<const u32x4*>(base + 16 * w) : u32x4{0, 0, 0, 0};
    }
}
// Unmasked whole words; a hull's first and last words may hold bytes of other
// frames (or headers): those are written byte by byte, the frame's own bytes
// only, so blocks of neighbouring frames never write the same byte.
template <int V>
__device__ __forceinline__ void store_piece(uint8_t* __restrict__ base, const kmws_desc& x, const PieceHull& h,
                                            const u32x4 (&v)[V])
{
    const uint32_t r = h.r;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const uint64_t w = h.w0 + threadIdx.x + (uint64_t)kBlock * i;
        if (w >= h.w1) continue;
        const uint64_t a = 16 * w;
        if (a >= x.off && a + 16 <= h.end) {
            *reinterpret_cast<u32x4*>(base + a) = v[i] ^ r;
        } else {  // the hull's first or last word: own bytes only
            const uint64_t lo = a > x.off ? a : x.off, hi = a + 16 < h.end ? a + 16 : h.end;
            for (uint64_t q = lo; q < hi; ++q) {
                const uint32_t b = (uint32_t)(q - a);
                const uint32_t dw = (b & 8u) ? ((b & 4u) ? v[i].w : v[i].z) : ((b & 4u) ? v[i].y : v[i].x);
                base[q] = (uint8_t)((dw ^ r) >> (8 * (b & 3u)));
            }
        }
    }
}

// Tile geometry used by the product path (tuned on MI355X).
constexpr int kUnmaskV = 4;
// Load depth of the capped launches (unmask_split_kernel<V, TWO = true, NT>):
// the payload loads a lane keeps outstanding.  kUnmaskV: all of a tile's loads
// go out up front.  Below it, a covered tile issues load i + depth when word i
// has arrived, ahead of word i's store; the other tile kinds issue the rest at
// once.  With kUnmaskBlocksPerCu (kmws_unmask.hip) it sets the payload bytes in
// flight per CU, blocks x depth x 4 KiB, picked as one pair by measurement:
// (3, 3), 36 KiB, ran the 64 GiB aligned batch at 20.18-20.39 ms against
// 20.59-20.74 for (2, 4) and 20.62-20.66 for (3, 4)
// (profiles/p04_unmask_depth_ab.txt).
constexpr int kUnmaskDepth = 3;
static_assert(kUnmaskDepth >= 1 && kUnmaskDepth <= kUnmaskV, "1 .. all of a tile's loads");
using ProdCfg = UnmaskCfg<kUnmaskV>;
constexpr uint32_t kUnmaskStaticLds = ProdCfg::kCap * (8 + 8 + 4);  // s_off, s_end, s_key

// ---- host side (kmws_unmask.hip) ----
// A schedule code of kmws_unmask_apply_sched, decoded once per call (false: not
// a valid code); default_schedule: the code of a batch nobody tuned.
struct Schedule {
    Split split;
    bool temporal;
};
bool decode_schedule(uint32_t code, Schedule* out);
uint32_t default_schedule(uint64_t span, uint32_t n);
// The apply's launches behind a launched plan (kmws_arena_place times them).
kmws_status launch_apply(const Schedule& sc, uint8_t* base, uint64_t span, const kmws_desc* descs, uint32_t n,
                         const void* workspace, size_t ws_bytes, hipStream_t s);
// The batch takes the capped launches (mean region of a tile or more: the one-
// and two-frame mask paths); the dynamic LDS a capped launch asks for so that
// exactly blocks_per_cu blocks with static_lds bytes of static LDS share a CU.
bool unmask_capped(uint64_t span, uint32_t n);
unsigned lds_pad_for(unsigned blocks_per_cu, unsigned static_lds);
// The full-tile grid of a payload pass: `nblocks` blocks in launches of at most
// 2^31 work-items (a launch may hold at most 2^32: huge spans go in pieces).
// Each slice goes to launch(std::bool_constant<TWO>, std::bool_constant<NT>,
// grid, b0, lds_pad) with the kernel's instantiation picked here: TWO = the
// capped launch (lds_pad != 0), NT = streaming stores (!temporal).
template <class Launch>
inline void launch_split_grid(uint64_t nblocks, unsigned lds_pad, bool temporal, Launch&& launch)
{
    constexpr uint64_t kMaxBlocks = (1ull << 32) / kBlock / 2;
    for (uint64_t b0 = 0; b0 < nblocks; b0 += kMaxBlocks) {
        const dim3 grid((uint32_t)(nblocks - b0 < kMaxBlocks ? nblocks - b0 : kMaxBlocks));
        const uint32_t bb = (uint32_t)b0;
        if (lds_pad && !temporal) launch(std::true_type{}, std::true_type{}, grid, bb, lds_pad);
        else if (lds_pad) launch(std::true_type{}, std::false_type{}, grid, bb, lds_pad);
        else if (!temporal) launch(std::false_type{}, std::true_type{}, grid, bb, 0u);
        else launch(std::false_type{}, std::false_type{}, grid, bb, 0u);
    }
}
// The first kernel of kmws_unpack_unmask: zeroes the workspace head, parses
// every header (out_desc / out_flags / out_err) and writes the unmask plan.
// The caller checked the arguments and the workspace size.
kmws_status launch_unpack_plan(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                               kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err, void* workspace,
                               hipStream_t s);

}  // namespace kmws
