// Tile loads and stores of the in-place payload passes (kmws_unmask.hip, and the
// fused unmask + UTF-8 pass of kmws_utf8.hip), and what the host side of those
// passes shares: the schedule codes and the occupancy cap of the apply.
#pragma once
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
// A schedule code of kmws_unmask_apply_sched is valid; it asks for temporal
// stores; the default of a batch nobody tuned.
bool valid_schedule(uint32_t code);
bool temporal_stores(uint32_t code);
uint32_t default_schedule(uint64_t span, uint32_t n);
// The batch takes the capped launches (mean region of a tile or more: the one-
// and two-frame mask paths); the dynamic LDS a capped launch asks for so that
// exactly blocks_per_cu blocks with static_lds bytes of static LDS share a CU.
bool unmask_capped(uint64_t span, uint32_t n);
unsigned lds_pad_for(unsigned blocks_per_cu, unsigned static_lds);
// The first kernel of kmws_unpack_unmask: zeroes the workspace head, parses
// every header (out_desc / out_flags / out_err) and writes the unmask plan.
// The caller checked the arguments and the workspace size.
kmws_status launch_unpack_plan(const uint8_t* wire, uint64_t wire_len, const uint64_t* hdr_off, uint32_t n, int mode,
                               kmws_desc* out_desc, uint16_t* out_flags, uint8_t* out_err, void* workspace,
                               hipStream_t s);

}  // namespace kmws
